"""dcvc_crc32_segments refuses a bad argument before any device work (crc32_validate): every call below passes
never-dereferenced device pointers on a box without a GPU, must return < 0 and must name the kernel in dcvc_last_error."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
P = 0x1000          # never dereferenced
P2 = 0x2000


def _call(base=P, offsets=(0,), lengths=(16,), n=None, out=P2, null_offsets=False, null_lengths=False):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_crc32_segments", ci, [vp, ctypes.POINTER(cll), ctypes.POINTER(cll), ci, vp, vp])
    off = None if null_offsets else (cll * max(1, len(offsets)))(*offsets)
    ln = None if null_lengths else (cll * max(1, len(lengths)))(*lengths)
    rc = f(vp(base) if base else None, off, ln, len(offsets) if n is None else n, vp(out) if out else None, None)
    return rc, _lib.lib().dcvc_last_error().decode()


REFUSED = [
    ("null base", dict(base=0)),
    ("null offsets", dict(null_offsets=True)),
    ("null lengths", dict(null_lengths=True)),
    ("null output", dict(out=0)),
    ("n = 0", dict(n=0)),
    ("n = -1", dict(n=-1)),
    ("n = 17", dict(offsets=(0,) * 17, lengths=(1,) * 17)),
    ("negative offset", dict(offsets=(-1,))),
    ("negative length", dict(lengths=(-16,))),
    ("negative offset in the last of 16", dict(offsets=(0,) * 15 + (-4,), lengths=(1,) * 16)),
    ("negative length in the second of 3", dict(offsets=(0, 16, 32), lengths=(16, -1, 16))),
    ("output at an odd address", dict(out=P2 + 1)),
    ("output 2-byte aligned", dict(out=P2 + 2)),
    ("offset + length overflows", dict(offsets=(2 ** 62,), lengths=(2 ** 62,))),
    ("a segment that ends above 2^44 bytes", dict(offsets=(2 ** 44,), lengths=(1,))),
]


@pytest.mark.parametrize("why,kwargs", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_refused_before_any_launch(why, kwargs):
    rc, err = _call(**kwargs)
    assert rc < 0, why
    assert err.startswith("crc32:"), err


def test_the_message_names_the_segment_and_the_bound():
    assert "segment 1" in _call(offsets=(0, 16, 32), lengths=(16, -1, 16))[1]
    assert "1..16" in _call(n=0)[1] and "got 17" in _call(offsets=(0,) * 17, lengths=(1,) * 17)[1]
    assert "4-byte aligned" in _call(out=P2 + 2)[1]
