"""Helpers for the -m gpu tests: typed ctypes access to the kernel-level C ABI
(include/dcvc_amd_ops.h) with torch tensors as device memory."""
import ctypes

import numpy as np
import torch

from dcvc_amd import _lib

vp, ci, cf, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


def _f(name, args):
    return _lib.fn(name, ci, args)


class Ops:
    def __init__(self):
        self.conv1x1 = _f("dcvc_conv1x1", [vp, ci, vp, vp, vp, ci, vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, vp])
        self.conv_kxk = _f("dcvc_conv_kxk", [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, ci, vp])
        self.tconv2x2 = _f("dcvc_tconv2x2", [vp, ci, vp, vp, ci, ci, ci, ci, ci, vp])
        self.dwconv3x3 = _f("dcvc_dwconv3x3", [vp, ci, vp, vp, ci, ci, ci, ci, vp])
        self.pad_unshuffle8 = _f("dcvc_pad_unshuffle8", [vp, ci, ci, ci, vp, ci, ci, vp])
        self.pad_unshuffle8_ld = _f("dcvc_pad_unshuffle8_ld", [vp, ci, ci, ci, vp, ci, ci, ci, vp])
        self.shuffle8 = _f("dcvc_shuffle8", [vp, ci, ci, ci, ci, ci, vp, vp])
        self.shuffle2 = _f("dcvc_shuffle2", [vp, ci, ci, ci, ci, vp, ci, vp])
        self.replicate_pad = _f("dcvc_replicate_pad", [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp])
        self.crop = _f("dcvc_crop", [vp, ci, ci, vp, ci, ci, ci, ci, vp])
        self.mul_channel = _f("dcvc_mul_channel", [vp, ci, vp, vp, ci, ci, ci, vp])
        self.round_z = _f("dcvc_round_z", [vp, vp, vp, ci, vp])
        self.int8_to_half = _f("dcvc_int8_to_half", [vp, vp, ci, vp])
        self.symbol_blocks = _f("dcvc_symbol_blocks", [ci])
        self.y_step_enc = _f("dcvc_y_step_enc", [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp,
                                                 ci, ci, ci, ci, cf, vp])
        self.y_step_dec_index = _f("dcvc_y_step_dec_index", [vp, ci, vp, vp, vp, vp, vp,
                                                             ci, ci, ci, ci, cf, vp])
        self.y_step_dec_restore = _f("dcvc_y_step_dec_restore", [vp, vp, vp, vp, vp, ci, vp, ci,
                                                                 ci, ci, ci, ci, vp])
        self.y_step_enc_b = _f("dcvc_y_step_enc_b", [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, cll, vp, ci, ci,
                                                     ci, ci, ci, ci, cf, ci, vp])
        self.y_step_dec_index_b = _f("dcvc_y_step_dec_index_b", [vp, ci, vp, vp, vp, vp, cll, vp, ci, ci,
                                                                 ci, ci, ci, ci, cf, ci, vp])
        self.y_step_dec_restore_b = _f("dcvc_y_step_dec_restore_b", [vp, cll, vp, vp, vp, ci, ci, vp, ci, vp, ci,
                                                                     ci, ci, ci, ci, ci, vp])
        self.mask_step_enc = _f("dcvc_mask_step_enc", [vp, ci, vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp,
                                                       ci, ci, ci, ci, ci, cf, vp])
        self.mask_dec_index = _f("dcvc_mask_dec_index", [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, cf, vp])
        self.mask_step_dec = _f("dcvc_mask_step_dec", [vp, vp, vp, vp, vp, vp, ci, vp, ci, vp, ci,
                                                       ci, ci, ci, ci, ci, vp])
        self.ffn_fused = _f("dcvc_ffn_fused", [vp, ci, vp, vp, vp, vp, vp, ci, vp, vp, vp, ci, ci, ci, ci, vp])
        self.dcb_tail = _f("dcvc_dcb_tail", [vp, vp, vp, ci, vp, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci,
                                             ci, ci, ci, ci, ci, ci, vp])
        self.dcb_nsplit = _f("dcvc_dcb_nsplit", [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci,
                                                 ci, ci, ci, ci, vp])
        self.dcb_nsplit_fin = _f("dcvc_dcb_nsplit_fin", [vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci, ci,
                                                         vp, ci, ci, ci, ci, ci, vp])
        self.dcb_nsplit_fin_supported = _f("dcvc_dcb_nsplit_fin_supported", [ci, ci, ci])
        self.dcb_nsplit_dw = _f("dcvc_dcb_nsplit_dw", [vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, ci,
                                                       vp, vp, vp, vp, ci, ci, vp, ci, ci, ci, ci, ci, vp])
        self.dcb_nsplit_dw_supported = _f("dcvc_dcb_nsplit_dw_supported", [ci, ci, ci])
        self.dcb_pair = _f("dcvc_dcb_pair", [vp, ci, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp])
        self.dcb_pair_supported = _f("dcvc_dcb_pair_supported", [ci, ci, ci])
        self.dcb_nsplit_pack = _f("dcvc_dcb_nsplit_pack", [vp, vp, vp, vp, ci, ci, vp, ctypes.POINTER(vp)])
        self.dcb_nsplit_packed = _f("dcvc_dcb_nsplit_packed", [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, ci, vp, ci,
                                                               ci, ci, ci, vp])
        self.dcb_nsplit_free = _f("dcvc_dcb_nsplit_free", [vp])
        self.scale_clamped = _f("dcvc_scale_clamped", [vp, ci, vp, ci, vp, ci, ci, ci, ci, vp])


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def call(fn, *args):
    _lib.check(fn(*args))


def nhwc(t):
    """[1, C, H, W] tensor -> contiguous [H, W, C]."""
    return t[0].permute(1, 2, 0).contiguous()


def nchw(t):
    """[H, W, C] -> [1, C, H, W]."""
    return t.permute(2, 0, 1).unsqueeze(0).contiguous()


# ---------------------------------------------------------------------------------------------- sentinels around outputs
SENT = 0x7E5A               # an fp16 NaN payload (the GEMM tests' sentinel)
SENT8 = 0x5A
SENT32 = 0x7E5A7E5A
_FILL = {torch.int16: SENT, torch.uint8: SENT8, torch.int8: SENT8, torch.int32: SENT32}


def at(t, elems=0):
    """pointer to element `elems` of a device tensor"""
    return ctypes.c_void_p(t.data_ptr() + elems * t.element_size())


def guarded(count, dtype, tail=16):
    """count elements and a tail behind them, all sentinel"""
    return torch.full((count + tail,), _FILL[dtype], dtype=dtype, device="cuda")


def tail_intact(t, count):
    return bool((t[count:] == _FILL[t.dtype]).all())


class Rows:
    """[pixels][C] halves on the device: dense, or a channel slice (16 bytes in) of a wider row whose other channels hold
    NaN-payload sentinels; one sentinel row behind the last pixel either way. a = None: `fill` = (pixels, value)."""

    def __init__(self, a, C, ld=None, fill=None):
        a = None if a is None else np.ascontiguousarray(a, dtype=np.float16).reshape(-1, C)
        self.C, self.ld = C, ld or C
        self.off = 8 if self.ld != C else 0
        assert self.off + C <= self.ld
        self.pixels = fill[0] if a is None else a.shape[0]
        self.buf = torch.full((self.pixels + 1, self.ld), SENT, dtype=torch.int16, device="cuda")
        if a is not None:
            self.view()[:] = torch.from_numpy(a.view(np.int16)).cuda()
        else:
            self.view()[:] = int(np.asarray(fill[1], np.float16).reshape(1).view(np.int16)[0])

    def view(self):
        return self.buf[:self.pixels, self.off:self.off + self.C]

    def ptr(self, pixel=0):
        return at(self.buf, pixel * self.ld + self.off)

    def get(self):
        return self.view().cpu().numpy().view(np.float16)

    def around_intact(self):
        b = self.buf
        return bool((b[:self.pixels, :self.off] == SENT).all() and (b[:self.pixels, self.off + self.C:] == SENT).all()
                    and (b[self.pixels:] == SENT).all())
