"""Capture and file layouts ("wire formats") on the GPU: NV21, NV16 / P210, UYVY, YUY2 / Y210 / Y216 and v210.

Thin wrappers over the C-ABI entry points ``dcvc_wire_carrier``, ``dcvc_wire_picture_bytes``, ``dcvc_wire_unpack`` and
``dcvc_wire_pack`` (include/dcvc_amd_ops.h). A wire picture is a flat ``torch.uint8`` CUDA tensor of ``picture_bytes`` bytes,
exactly the file's; its carrier is one picture in the file layout of ``carrier(wire)`` as ``pixfmt.to_x`` takes it and
``pixfmt.from_x`` returns it: ``torch.uint8`` at 8 bits, 16-bit samples above (LSB-aligned for YUV422P). The kernels run on
``torch.cuda.current_stream()``.

  nv21   Y [H][W], then [H/2][W/2][2] as Cr, Cb; 8 bits; carrier NV12
  nv16   Y [H][W], then [H][W/2][2] as Cb, Cr; 8 bits, or 9..16: u16 with the value in the high bits (P210); carrier YUV422P
  uyvy   [H][W/2] x (Cb, Y0, Cr, Y1); 8 bits; carrier YUV422P
  yuy2   [H][W/2] x (Y0, Cb, Y1, Cr); 8 bits, or 9..16: u16 with the value in the high bits (Y210 / Y212 / Y216); carrier YUV422P
  v210   rows of 128 ceil(W / 48) bytes, 6 pixels in four 32-bit words of three 10-bit fields; 10 bits; carrier YUV422P
"""
import ctypes

from . import _lib
from .pixfmt import picture_samples
from .yuv16 import _u16_dtypes, u16_dtype

DCVC_WIRE_NV21 = 0
DCVC_WIRE_NV16 = 1
DCVC_WIRE_UYVY = 2
DCVC_WIRE_YUY2 = 3
DCVC_WIRE_V210 = 4
WIRE = {"nv21": DCVC_WIRE_NV21, "nv16": DCVC_WIRE_NV16, "uyvy": DCVC_WIRE_UYVY, "yuy2": DCVC_WIRE_YUY2, "v210": DCVC_WIRE_V210}

_vp, _ci, _ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
_fns = {}
_SIGS = {
    "dcvc_wire_carrier": (_ci, [_ci]),
    "dcvc_wire_picture_bytes": (_ll, [_ci, _ci, _ci, _ci]),
    "dcvc_wire_unpack": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp]),
    "dcvc_wire_pack": (_ci, [_vp, _ci, _ci, _ci, _ci, _vp, _vp]),
}


def _fn(name):
    if name not in _fns:
        _fns[name] = _lib.fn(name, *_SIGS[name])
    return _fns[name]


def _stream(t):
    import torch
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


def carrier(wire):
    """the DCVC_PIX_* layout that holds the wire format's samples"""
    return _lib.check(_fn("dcvc_wire_carrier")(wire))


def picture_bytes(wire, bit_depth, H, W):
    """file bytes of one wire picture"""
    return _lib.check(_fn("dcvc_wire_picture_bytes")(wire, bit_depth, H, W))


def unpack(src, wire, bit_depth, H, W):
    """One wire picture (flat uint8 CUDA tensor of picture_bytes bytes) -> its carrier picture, a flat tensor of
    pixfmt.picture_samples(carrier(wire), H, W) samples as pixfmt.to_x takes it (uint8, or u16_dtype() above 8 bits)."""
    import torch
    n = picture_bytes(wire, bit_depth, H, W)
    if src.dtype != torch.uint8 or not src.is_cuda or not src.is_contiguous() or src.numel() != n:
        raise ValueError("unpack: a contiguous CUDA uint8 tensor of %d bytes expected, got %d of %s" % (n, src.numel(), src.dtype))
    out = torch.empty(picture_samples(carrier(wire), H, W), dtype=torch.uint8 if bit_depth == 8 else torch.int16, device=src.device)
    _lib.check(_fn("dcvc_wire_unpack")(_vp(src.data_ptr()), wire, bit_depth, H, W, _vp(out.data_ptr()), _stream(src)))
    return out if bit_depth == 8 else out.view(u16_dtype())


def pack(carrier_picture, wire, bit_depth, H, W):
    """One carrier picture (as unpack returns it; int16 storage is read as unsigned) -> the wire picture, a flat uint8 tensor
    of picture_bytes bytes with every byte defined."""
    import torch
    n = picture_bytes(wire, bit_depth, H, W)
    c = carrier_picture
    samples = picture_samples(carrier(wire), H, W)
    dtypes = (torch.uint8,) if bit_depth == 8 else _u16_dtypes()
    if c.dtype not in dtypes or not c.is_cuda or not c.is_contiguous() or c.numel() != samples:
        raise ValueError("pack: a contiguous CUDA tensor of %d %s samples expected, got %d of %s"
                         % (samples, "uint8" if bit_depth == 8 else "uint16 / int16", c.numel(), c.dtype))
    out = torch.empty(n, dtype=torch.uint8, device=c.device)
    _lib.check(_fn("dcvc_wire_pack")(_vp(c.data_ptr()), wire, bit_depth, H, W, _vp(out.data_ptr()), _stream(c)))
    return out


__all__ = ["DCVC_WIRE_NV21", "DCVC_WIRE_NV16", "DCVC_WIRE_UYVY", "DCVC_WIRE_YUY2", "DCVC_WIRE_V210", "WIRE", "carrier",
           "picture_bytes", "unpack", "pack"]
