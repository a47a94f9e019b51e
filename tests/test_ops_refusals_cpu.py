"""The layout, elementwise and symbol entry points of the kernel-level C ABI refuse a bad argument before any device work:
every call below passes never-dereferenced pointers on a box without a GPU, must return < 0 and must name its entry point in
dcvc_last_error. Single and batched forms share their checks (capi_ops.hip), so each refusal is tried on both."""
import ctypes

import pytest

vp, ci, cf, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
P = vp(0x1000)          # never dereferenced
P2 = vp(0x2000)
ODD = vp(0x1008)        # not 16-byte aligned
NULL = None


def _fn(name, args):
    from dcvc_amd import _lib
    return _lib.fn("dcvc_" + name, ci, args)


def _err():
    from dcvc_amd import _lib
    return _lib.lib().dcvc_last_error().decode()


SIG = {
    "pad_unshuffle8": [vp, ci, ci, ci, vp, ci, ci, vp],
    "pad_unshuffle8_ld": [vp, ci, ci, ci, vp, ci, ci, ci, vp],
    "pad_unshuffle8_b": [vp, ci, ci, ci, vp, ci, ci, ci, vp],
    "shuffle8": [vp, ci, ci, ci, ci, ci, vp, vp],
    "shuffle8_b": [vp, ci, ci, ci, ci, ci, vp, ci, vp],
    "shuffle2": [vp, ci, ci, ci, ci, vp, ci, vp],
    "replicate_pad": [vp, ci, ci, ci, ci, ci, ci, vp, ci, vp],
    "replicate_pad_b": [vp, ci, ci, ci, ci, ci, ci, vp, ci, ci, vp],
    "crop": [vp, ci, ci, vp, ci, ci, ci, ci, vp],
    "crop_b": [vp, ci, ci, ci, vp, ci, ci, ci, ci, ci, vp],
    "mul_channel": [vp, ci, vp, vp, ci, ci, ci, vp],
    "scale_clamped": [vp, ci, vp, ci, vp, ci, ci, ci, ci, vp],
    "round_z": [vp, vp, vp, ci, vp],
    "int8_to_half": [vp, vp, ci, vp],
    "y_step_enc": [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, vp],
    "y_step_enc_b": [vp, ci, vp, ci, vp, ci, vp, ci, vp, vp, vp, vp, cll, vp, ci, ci, ci, ci, ci, ci, cf, ci, vp],
    "y_step_dec_index": [vp, ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, cf, vp],
    "y_step_dec_index_b": [vp, ci, vp, vp, vp, vp, cll, vp, ci, ci, ci, ci, ci, ci, cf, ci, vp],
    "y_step_dec_restore": [vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci, ci, vp],
    "y_step_dec_restore_b": [vp, cll, vp, vp, vp, ci, ci, vp, ci, vp, ci, ci, ci, ci, ci, ci, vp],
}


def _enc(y=P, ldy=64, lds=64, ldm=64, acc=P2, ldacc=64, sym=P, H=4, W=4, C=64, step=0):
    return (y, ldy, P, lds, P, ldm, acc, ldacc, sym, P, P, P, P, H, W, C, step, 0.15, NULL)


def _enc_b(y=P, ldy=64, sym=P, out_stride=1024, totals_stride=4, slot=0, H=4, W=4, C=64, step=0, n=2):
    return (y, ldy, P, 64, P, 64, P2, 64, sym, P, P, P, out_stride, P, totals_stride, slot, H, W, C, step, 0.15, n, NULL)


def _idx(scales=P, lds=64, index=P, H=4, W=4, C=64, step=0):
    return (scales, lds, index, P, P, P, P, H, W, C, step, 0.15, NULL)


def _idx_b(scales=P, lds=64, out_stride=1024, totals_stride=260, slot=0, C=64, step=0, n=2):
    return (scales, lds, P, P, P, P, out_stride, P, totals_stride, slot, 4, 4, C, step, 0.15, n, NULL)


def _res(decoded=P, means=P, ldm=64, acc=P2, ldacc=64, H=4, W=4, C=64, step=0):
    return (decoded, P, P, P, means, ldm, acc, ldacc, H, W, C, step, NULL)


def _res_b(decoded_stride=1024, totals_stride=260, slot=0, means=P, ldm=64, C=64, step=0, n=2):
    return (P, decoded_stride, P, P, P, totals_stride, slot, means, ldm, P2, 64, 4, 4, C, step, n, NULL)


# (entry point, arguments, what is wrong with them)
REFUSED = [
    # ---- layout: null pointers, sizes, C % 8, ld < C, 16-byte accesses, padding, output size
    ("pad_unshuffle8", (NULL, 16, 16, 3, P, 2, 2, NULL), "null input"),
    ("pad_unshuffle8", (P, 16, 16, 3, NULL, 2, 2, NULL), "null output"),
    ("pad_unshuffle8", (P, 0, 16, 3, P, 2, 2, NULL), "no rows"),
    ("pad_unshuffle8", (P, 17, 16, 3, P, 2, 2, NULL), "2 x 8 rows < 17"),
    ("pad_unshuffle8", (P, 16, 17, 3, P, 2, 2, NULL), "2 x 8 columns < 17"),
    ("pad_unshuffle8", (P, 16, 16, 3, ODD, 2, 2, NULL), "misaligned output"),
    ("pad_unshuffle8_ld", (P, 16, 16, 3, P, 191, 2, 2, NULL), "ldout below 64 * C3"),
    ("pad_unshuffle8_ld", (P, 16, 16, 3, P, 196, 2, 2, NULL), "ldout no multiple of 8"),
    ("pad_unshuffle8_ld", (P, 16, 16, 3, ODD, 200, 2, 2, NULL), "misaligned output"),
    ("pad_unshuffle8_ld", (P, 16, 16, 0, P, 200, 2, 2, NULL), "no channels"),
    ("pad_unshuffle8_ld", (P, 17, 16, 3, P, 200, 2, 2, NULL), "2 x 8 rows < 17"),
    ("pad_unshuffle8_ld", (NULL, 16, 16, 3, P, 200, 2, 2, NULL), "null input"),
    ("pad_unshuffle8_b", (P, 16, 16, 3, ODD, 2, 2, 2, NULL), "misaligned output"),
    ("shuffle8", (NULL, 192, 2, 2, 3, 1, P, NULL), "null input"),
    ("shuffle8", (P, 191, 2, 2, 3, 1, P, NULL), "ldin below 64 * C3"),
    ("shuffle8", (P, 196, 2, 2, 3, 1, P, NULL), "ldin no multiple of 8"),
    ("shuffle8", (ODD, 192, 2, 2, 3, 1, P, NULL), "misaligned input"),
    ("shuffle8", (P, 192, 2, -2, 3, 1, P, NULL), "negative width"),
    ("shuffle8_b", (ODD, 192, 2, 2, 3, 1, P, 2, NULL), "misaligned input"),
    ("shuffle8_b", (P, 196, 2, 2, 3, 1, P, 2, NULL), "ldin no multiple of 8"),
    ("shuffle2", (NULL, 64, 4, 4, 16, P, 16, NULL), "null input"),
    ("shuffle2", (P, 64, 4, 4, 20, P, 24, NULL), "C = 20"),
    ("shuffle2", (P, 63, 4, 4, 16, P, 16, NULL), "ldin below 4 C"),
    ("shuffle2", (P, 64, 4, 4, 16, P, 8, NULL), "ldout below C"),
    ("shuffle2", (P, 64, 4, 4, 16, P, 20, NULL), "ldout no multiple of 8"),
    ("shuffle2", (P, 64, 4, 4, 16, ODD, 16, NULL), "misaligned output"),
    ("shuffle2", (P, 64, 0, 4, 16, P, 16, NULL), "no rows"),
    ("replicate_pad", (NULL, 32, 4, 4, 32, 1, 1, P, 32, NULL), "null input"),
    ("replicate_pad", (P, 32, 4, 4, 32, -1, 0, P, 32, NULL), "negative padding"),
    ("replicate_pad", (P, 32, 4, 4, 32, 0, -1, P, 32, NULL), "negative padding"),
    ("replicate_pad", (P, 32, 4, 4, 20, 0, 0, P, 32, NULL), "C = 20"),
    ("replicate_pad", (P, 24, 4, 4, 32, 0, 0, P, 32, NULL), "ldin below C"),
    ("replicate_pad", (P, 32, 4, 4, 32, 0, 0, P, 24, NULL), "ldout below C"),
    ("replicate_pad", (P, 36, 4, 4, 32, 0, 0, P, 32, NULL), "ldin no multiple of 8"),
    ("replicate_pad", (P, 32, 4, 4, 32, 0, 0, ODD, 32, NULL), "misaligned output"),
    ("replicate_pad_b", (P, 36, 4, 4, 32, 0, 0, P, 32, 2, NULL), "ldin no multiple of 8"),
    ("replicate_pad_b", (ODD, 32, 4, 4, 32, 0, 0, P, 32, 2, NULL), "misaligned input"),
    ("crop", (NULL, 32, 8, P, 32, 4, 4, 32, NULL), "null input"),
    ("crop", (P, 32, 3, P, 32, 4, 4, 32, NULL), "wider than its input"),
    ("crop", (P, 32, 8, P, 32, 4, 4, 20, NULL), "C = 20"),
    ("crop", (P, 24, 8, P, 32, 4, 4, 32, NULL), "ldin below C"),
    ("crop", (P, 32, 8, P, 36, 4, 4, 32, NULL), "ldout no multiple of 8"),
    ("crop", (ODD, 32, 8, P, 32, 4, 4, 32, NULL), "misaligned input"),
    ("crop", (P, 32, 8, P, 32, 0, 4, 32, NULL), "no rows"),
    ("crop_b", (P, 32, 8, 8, P, 36, 4, 4, 32, 2, NULL), "ldout no multiple of 8"),
    ("crop_b", (P, 32, 8, 8, ODD, 32, 4, 4, 32, 2, NULL), "misaligned output"),
    # ---- elementwise
    ("mul_channel", (NULL, 32, P, P, 32, 8, 32, NULL), "null input"),
    ("mul_channel", (P, 32, NULL, P, 32, 8, 32, NULL), "null factors"),
    ("mul_channel", (P, 32, P, P, 32, 8, 20, NULL), "C = 20: the kernel would process 16 channels"),
    ("mul_channel", (P, 24, P, P, 32, 8, 32, NULL), "ldx below C"),
    ("mul_channel", (P, 32, P, P, 36, 8, 32, NULL), "ldy no multiple of 8"),
    ("mul_channel", (P, 32, ODD, P, 32, 8, 32, NULL), "misaligned factors"),
    ("mul_channel", (P, 32, P, P, 32, 0, 32, NULL), "no pixels"),
    ("scale_clamped", (P, 32, P, 32, NULL, 32, 8, 32, 0, NULL), "null output"),
    ("scale_clamped", (P, 32, P, 32, P, 32, 8, 20, 1, NULL), "C = 20"),
    ("scale_clamped", (P, 32, P, 24, P, 32, 8, 32, 1, NULL), "ldq below C"),
    ("scale_clamped", (P, 32, P, 36, P, 32, 8, 32, 0, NULL), "ldq no multiple of 8"),
    ("scale_clamped", (P, 32, ODD, 32, P, 32, 8, 32, 0, NULL), "misaligned q"),
    ("round_z", (NULL, P, P, 8, NULL), "null input"),
    ("round_z", (P, P, NULL, 8, NULL), "null int8 output"),
    ("round_z", (P, P, P, 0, NULL), "nothing to do"),
    ("round_z", (P, P, P, -8, NULL), "negative count"),
    ("round_z", (vp(0x1001), P, P, 8, NULL), "misaligned halves"),
    ("int8_to_half", (NULL, P, 8, NULL), "null input"),
    ("int8_to_half", (P, NULL, 8, NULL), "null output"),
    ("int8_to_half", (P, P, 0, NULL), "nothing to do"),
    ("int8_to_half", (P, vp(0x1001), 8, NULL), "misaligned halves"),
    # ---- the 4-step symbol kernels
    ("y_step_enc", _enc(y=NULL), "null latent"),
    ("y_step_enc", _enc(acc=NULL), "null y_hat"),
    ("y_step_enc", _enc(C=40, ldy=40, lds=40, ldm=40, ldacc=40), "C = 40: no multiple of 32"),
    ("y_step_enc", _enc(ldy=32), "ldy below C"),
    ("y_step_enc", _enc(ldacc=68), "ldacc no multiple of 8"),
    ("y_step_enc", _enc(y=ODD), "misaligned latent"),
    ("y_step_enc", _enc(sym=ODD), "misaligned symbols"),
    ("y_step_enc", _enc(H=0), "no rows"),
    ("y_step_enc", _enc(step=4), "step 4"),
    ("y_step_enc_b", _enc_b(n=0), "n = 0"),
    ("y_step_enc_b", _enc_b(n=17), "n = 17"),
    ("y_step_enc_b", _enc_b(y=NULL), "null latent"),
    ("y_step_enc_b", _enc_b(C=40), "C = 40"),
    ("y_step_enc_b", _enc_b(ldy=32), "ldy below C"),
    ("y_step_enc_b", _enc_b(sym=ODD), "misaligned symbols"),
    ("y_step_enc_b", _enc_b(out_stride=0), "pictures on top of each other"),
    ("y_step_enc_b", _enc_b(totals_stride=-4), "negative totals stride"),
    ("y_step_enc_b", _enc_b(slot=4), "slot 4"),
    ("y_step_dec_index", _idx(scales=NULL), "null scales"),
    ("y_step_dec_index", _idx(C=40, lds=40), "C = 40"),
    ("y_step_dec_index", _idx(lds=32), "lds below C"),
    ("y_step_dec_index", _idx(scales=ODD), "misaligned scales"),
    ("y_step_dec_index", _idx(index=vp(0x1004)), "misaligned indexes"),
    ("y_step_dec_index", _idx(W=-1), "negative width"),
    ("y_step_dec_index_b", _idx_b(n=0), "n = 0"),
    ("y_step_dec_index_b", _idx_b(C=40), "C = 40"),
    ("y_step_dec_index_b", _idx_b(lds=68), "lds no multiple of 8"),
    ("y_step_dec_index_b", _idx_b(totals_stride=0), "pictures share their totals"),
    ("y_step_dec_index_b", _idx_b(step=-1), "step -1"),
    ("y_step_dec_restore", _res(decoded=NULL), "null symbols"),
    ("y_step_dec_restore", _res(C=40, ldm=40, ldacc=40), "C = 40: refused nowhere before"),
    ("y_step_dec_restore", _res(C=8, ldm=8, ldacc=8), "C = 8"),
    ("y_step_dec_restore", _res(ldm=32), "ldm below C"),
    ("y_step_dec_restore", _res(means=ODD), "misaligned means"),
    ("y_step_dec_restore", _res(ldacc=68), "ldacc no multiple of 8"),
    ("y_step_dec_restore", _res(H=0), "no rows"),
    ("y_step_dec_restore_b", _res_b(n=17), "n = 17"),
    ("y_step_dec_restore_b", _res_b(C=40), "C = 40"),
    ("y_step_dec_restore_b", _res_b(means=NULL), "null means"),
    ("y_step_dec_restore_b", _res_b(decoded_stride=0), "pictures share their symbols"),
    ("y_step_dec_restore_b", _res_b(slot=-1), "slot -1"),
]


@pytest.mark.parametrize("name,args,why", REFUSED, ids=["%s-%s" % (r[0], r[2].replace(" ", "_")) for r in REFUSED])
def test_refused_before_any_launch(name, args, why):
    f = _fn(name, SIG[name])
    assert len(args) == len(SIG[name])
    assert f(*args) < 0, why
    assert _err().startswith(name + ":"), _err()


def test_every_entry_point_of_the_group_is_tried():
    assert {r[0] for r in REFUSED} == set(SIG)
