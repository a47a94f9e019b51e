"""dcvc_deinterlace_planes refuses a bad argument before any device work (deinterlace_validate): every call below
passes never-dereferenced device pointers on a box without a GPU, must return < 0 and must name the kernel in dcvc_last_error.
And dcvc_y4m_parse_header_i: the Y4M header entry that reports field-interlaced material instead of refusing it."""
import ctypes

import pytest

vp, ci, cll = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
U8, F16, U16, F32 = 0, 1, 3, 4
CUR, PREV, DST = 0x100000, 0x200000, 0x300000          # never dereferenced; 1 MiB apart


def _call(cur=CUR, crs=64, cps=64 * 48, prev=PREV, prs=64, pps=64 * 48, dst=DST, drs=64, dps=64 * 48, dtype=U8, bit_depth=8, H=48, W=64,
          n_planes=1, keep=0, weave=0, threshold=10):
    from dcvc_amd import _lib
    f = _lib.fn("dcvc_deinterlace_planes", ci, [vp, ci, cll, vp, ci, cll, vp, ci, cll, ci, ci, ci, ci, ci, ci, ci, ci, vp])
    rc = f(vp(cur) if cur else None, crs, cps, vp(prev) if prev else None, prs, pps, vp(dst) if dst else None, drs, dps, dtype, bit_depth,
           H, W, n_planes, keep, weave, threshold, None)
    return rc, _lib.lib().dcvc_last_error().decode()


REFUSED = [
    ("null cur", dict(cur=0), "null operand"),
    ("null dst", dict(dst=0), "null operand"),
    ("fp16 samples", dict(dtype=F16), "sample type"),
    ("fp32 samples", dict(dtype=F32), "sample type"),
    ("sample type 2", dict(dtype=2), "sample type"),
    ("sample type -1", dict(dtype=-1), "sample type"),
    ("u8 at 10 bits", dict(bit_depth=10), "bit_depth must be 8 (u8) or 9..16 (u16), got 10"),
    ("u8 at 7 bits", dict(bit_depth=7), "got 7"),
    ("u16 at 8 bits", dict(dtype=U16, bit_depth=8), "got 8"),
    ("u16 at 17 bits", dict(dtype=U16, bit_depth=17), "got 17"),
    ("H = 1", dict(H=1), "H must be in 2..16384"),
    ("H = 0", dict(H=0), "H must be in 2..16384"),
    ("H = -1", dict(H=-1), "H must be in 2..16384"),
    ("H = 16385", dict(H=16385), "H must be in 2..16384"),
    ("W = 0", dict(W=0), "W in 1..16384"),
    ("W = 16385", dict(W=16385, crs=16385, prs=16385, drs=16385), "W in 1..16384"),
    ("n_planes = 0", dict(n_planes=0), "n_planes must be in 1..65535"),
    ("n_planes = 65536", dict(n_planes=65536), "n_planes must be in 1..65535"),
    ("keep = 2", dict(keep=2), "keep must be 0 or 1, got 2"),
    ("keep = -1", dict(keep=-1), "keep must be 0 or 1, got -1"),
    ("weave_from_prev = 2", dict(weave=2), "weave_from_prev must be 0 or 1, got 2"),
    ("weave_from_prev = -1", dict(weave=-1), "weave_from_prev must be 0 or 1, got -1"),
    ("threshold = -1", dict(threshold=-1), "threshold must be in 0..64, got -1"),
    ("threshold = 65", dict(threshold=65), "threshold must be in 0..64, got 65"),
    ("cur row stride below W", dict(crs=63), "a row stride is below the width"),
    ("prev row stride below W", dict(prs=63), "a row stride is below the width"),
    ("dst row stride below W", dict(drs=63), "a row stride is below the width"),
    ("cur plane stride below the plane", dict(n_planes=2, cps=64 * 48 - 1), "a plane stride is below the plane"),
    ("prev plane stride below the plane", dict(n_planes=2, pps=64 * 48 - 1), "a plane stride is below the plane"),
    ("dst plane stride below the plane", dict(n_planes=2, dps=64 * 48 - 1), "a plane stride is below the plane"),
    ("u16 cur at an odd address", dict(dtype=U16, bit_depth=10, cur=CUR + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 prev at an odd address", dict(dtype=U16, bit_depth=10, prev=PREV + 1), "16-bit planes must be 2-byte aligned"),
    ("u16 dst at an odd address", dict(dtype=U16, bit_depth=10, dst=DST + 1), "16-bit planes must be 2-byte aligned"),
    ("dst is cur", dict(dst=CUR), "dst overlaps cur"),
    ("dst starts inside cur", dict(dst=CUR + 64 * 48 - 1), "dst overlaps cur"),
    ("dst ends inside cur", dict(dst=CUR - 64 * 48 + 1), "dst overlaps cur"),
    ("dst is prev", dict(dst=PREV), "dst overlaps prev"),
    ("dst starts inside prev's second plane", dict(n_planes=2, dst=PREV + 2 * 64 * 48 - 1), "dst overlaps prev"),
]


@pytest.mark.parametrize("why,kwargs,words", REFUSED, ids=[r[0].replace(" ", "_") for r in REFUSED])
def test_refused_before_any_launch(why, kwargs, words):
    rc, err = _call(**kwargs)
    assert rc < 0, why
    assert err.startswith("deinterlace:") and words in err, err


def test_prev_strides_are_not_read_without_prev():
    # strides that are refused with prev pass without it: the call gets as far as the overlap check, which comes last
    rc, err = _call(prev=0, prs=0, pps=0, n_planes=2, dst=CUR)
    assert rc < 0 and "overlaps cur" in err, err


def test_plane_strides_are_not_read_for_one_plane():
    rc, err = _call(cps=0, pps=0, dps=0, dst=CUR)
    assert rc < 0 and "overlaps cur" in err, err


# ------------------------------------------------------------------------------------ Y4M
def _header(fields):
    return ("YUV4MPEG2 W352 H288 F25:1 %s\nFRAME\n" % fields).strip(" ").encode().replace(b"  ", b" ")


@pytest.mark.parametrize("field,want", [("Ip", 0), ("I?", 0), ("", 0), ("It", 1), ("Ib", 2)])
def test_parse_header_i_reports_the_field_order(field, want):
    from dcvc_amd import pixfmt
    data = _header((field + " C422p10").strip())
    info = pixfmt.y4m_header_i(data)
    assert info["interlacing"] == want
    assert (info["width"], info["height"], info["pix_fmt"], info["bit_depth"]) == (352, 288, pixfmt.DCVC_PIX_YUV422P, 10)
    assert info["header_bytes"] == data.index(b"\n") + 1
    if want == 0:
        plain = pixfmt.y4m_header(data)
        assert all(plain[k] == info[k] for k in plain)


def test_mixed_interlacing_stays_refused():
    from dcvc_amd import _lib, pixfmt
    with pytest.raises(_lib.DcvcError, match="field Im: interlaced material is not supported"):
        pixfmt.y4m_header_i(_header("Im"))
    with pytest.raises(_lib.DcvcError, match="unknown field"):
        pixfmt.y4m_header_i(_header("It Q1"))


def test_the_old_entry_refuses_interlaced_files_with_the_old_words():
    from dcvc_amd import _lib, pixfmt
    for field in ("It", "Ib", "Im"):
        with pytest.raises(_lib.DcvcError, match="field %s: interlaced material is not supported" % field):
            pixfmt.y4m_header(_header(field))
    assert pixfmt.y4m_header(_header("Ip"))["width"] == 352


def test_parse_header_i_needs_its_arguments():
    from dcvc_amd import _lib
    from dcvc_amd.pixfmt import Y4mInfo
    f = _lib.fn("dcvc_y4m_parse_header_i", ci, [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(Y4mInfo), ctypes.POINTER(ci)])
    data = _header("It")
    assert f(data, len(data), ctypes.byref(Y4mInfo()), None) < 0
    assert "null argument" in _lib.lib().dcvc_last_error().decode()
