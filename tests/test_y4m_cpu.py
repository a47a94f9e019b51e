"""YUV4MPEG2 headers (csrc/image/y4m.cpp through dcvc_amd.pixfmt): every accepted chroma tag, field order, a missing C, FRAME
lines with parameters, the write-then-parse round trip and every refusal, each naming the offending field. Host code only."""
import pytest

from dcvc_amd import pixfmt
from dcvc_amd._lib import DcvcError

P420, P422, P444, NV12 = pixfmt.DCVC_PIX_YUV420P, pixfmt.DCVC_PIX_YUV422P, pixfmt.DCVC_PIX_YUV444P, pixfmt.DCVC_PIX_NV12

TAGS = [("420jpeg", P420, 8), ("420mpeg2", P420, 8), ("420paldv", P420, 8), ("420", P420, 8), ("422", P422, 8), ("444", P444, 8)] + \
       [("%sp%d" % (b, n), f, n) for b, f in (("420", P420), ("422", P422), ("444", P444)) for n in range(9, 17)]


@pytest.mark.parametrize("tag,fmt,bits", TAGS, ids=[t[0] for t in TAGS])
def test_accepted_tags(tag, fmt, bits):
    head = b"YUV4MPEG2 W352 H288 F30000:1001 Ip A128:117 C%s XYSCSS=%s\n" % (tag.encode(), tag.upper().encode())
    h = pixfmt.y4m_header(head + b"FRAME\n" + bytes(64))
    assert h == dict(width=352, height=288, fps_num=30000, fps_den=1001, pix_fmt=fmt, bit_depth=bits, header_bytes=len(head))


def test_field_order_missing_fields_and_defaults():
    a = pixfmt.y4m_header(b"YUV4MPEG2 C444p10 Ip H96 XCOLORRANGE=LIMITED F25:1 W128 A1:1\nFRAME\n")
    assert (a["width"], a["height"], a["pix_fmt"], a["bit_depth"], a["fps_num"], a["fps_den"]) == (128, 96, P444, 10, 25, 1)
    b = pixfmt.y4m_header(b"YUV4MPEG2 W128 H96\n")                       # no C: 4:2:0 at 8 bits; no F: 25:1; no I: progressive
    assert (b["pix_fmt"], b["bit_depth"], b["fps_num"], b["fps_den"], b["header_bytes"]) == (P420, 8, 25, 1, 19)
    c = pixfmt.y4m_header(b"YUV4MPEG2 W128 H96 I? F0:0  C422\n")         # I?, an unknown rate, two spaces
    assert (c["pix_fmt"], c["fps_num"], c["fps_den"]) == (P422, 25, 1)
    long_comment = b"YUV4MPEG2 W128 H96 X" + b"c" * 900 + b" C444\n"
    assert pixfmt.y4m_header(long_comment)["pix_fmt"] == P444 and len(long_comment) < 1024


def test_frame_lines():
    assert pixfmt.y4m_frame_header_bytes(b"FRAME\n" + bytes(8)) == 6
    assert pixfmt.y4m_frame_header_bytes(b"FRAME Ip Xabc\n\n\n") == 14
    for bad in (b"", b"FRAME", b"FRAMES\n", b"frame\n", b"YUV4MPEG2 W2 H2\n", b"FRAME " + b"x" * 2000 + b"\n"):
        with pytest.raises(DcvcError, match="^y4m_frame_header_bytes: "):
            pixfmt.y4m_frame_header_bytes(bad)


@pytest.mark.parametrize("fmt,bits,tag", [(P420, 8, b"C420jpeg"), (P420, 10, b"C420p10"), (P422, 8, b"C422"), (P422, 10, b"C422p10"),
                                          (P444, 8, b"C444"), (P444, 16, b"C444p16")])
def test_write_then_parse(fmt, bits, tag):
    head = pixfmt.y4m_write_header(1920, 1080, fmt, bits, 60000, 1001)
    assert head.startswith(b"YUV4MPEG2 ") and head.endswith(b" " + tag + b"\n") and head.count(b"\n") == 1
    h = pixfmt.y4m_header(head)
    assert h == dict(width=1920, height=1080, fps_num=60000, fps_den=1001, pix_fmt=fmt, bit_depth=bits, header_bytes=len(head))


def test_writer_refusals():
    for args in ((1920, 1080, NV12, 8), (1920, 1080, NV12, 10), (1920, 1081, P420, 8), (0, 1080, P420, 8), (1920, 1080, P420, 7),
                 (1920, 1080, P420, 17), (1920, 1080, P444, 8, 0, 1), (1920, 1080, P444, 8, 25, 0), (1920, 1080, 7, 8)):
        with pytest.raises(DcvcError, match="^y4m_write_header: "):
            pixfmt.y4m_write_header(*args)


REFUSED = [
    (b"YUV4MPEG2 W128 H96 It\n", "It"), (b"YUV4MPEG2 W128 H96 Ib C420\n", "Ib"), (b"YUV4MPEG2 Im W128 H96\n", "Im"),
    (b"YUV4MPEG2 W128 H96 Cmono\n", "Cmono"), (b"YUV4MPEG2 W128 H96 Cmono16\n", "Cmono16"), (b"YUV4MPEG2 W128 H96 C411\n", "C411"),
    (b"YUV4MPEG2 W128 H96 C444alpha\n", "C444alpha"), (b"YUV4MPEG2 W128 H96 C440\n", "C440"), (b"YUV4MPEG2 W128 H96 C420p8\n", "C420p8"),
    (b"YUV4MPEG2 W128 H96 C444p17\n", "C444p17"), (b"YUV4MPEG2 W128 H96 C422p\n", "C422p"), (b"YUV4MPEG2 W128 H96 C420jpegp10\n", "C420jpegp10"),
    (b"YUV4MPEG2 W0 H96\n", "W0"), (b"YUV4MPEG2 W128 H-96\n", "H-96"), (b"YUV4MPEG2 W127 H96\n", "W127"), (b"YUV4MPEG2 W128 H95 C444\n", "H95"),
    (b"YUV4MPEG2 W128 Hx\n", "Hx"), (b"YUV4MPEG2 H96\n", "no W field"), (b"YUV4MPEG2 W128 C444\n", "no H field"),
    (b"YUV4MPEG2 W128 H96 F25\n", "F25"), (b"YUV4MPEG2 W128 H96 Q1\n", "Q1"),
]


@pytest.mark.parametrize("head,names", REFUSED, ids=[r[1].replace(" ", "_") for r in REFUSED])
def test_refused_headers_name_the_field(head, names):
    with pytest.raises(DcvcError) as e:
        pixfmt.y4m_header(head + b"FRAME\n")
    assert str(e.value).startswith("y4m_parse_header: ") and names in str(e.value), str(e.value)


def test_not_a_y4m_file():
    for bad in (b"", b"YUV4MPEG", b"YUV4MPEG3 W2 H2\n", b"yuv4mpeg2 W2 H2\n", bytes(64), b"YUV4MPEG2W2 H2\n"):
        with pytest.raises(DcvcError, match="no YUV4MPEG2 magic"):
            pixfmt.y4m_header(bad)
    with pytest.raises(DcvcError, match="no end of the header line"):
        pixfmt.y4m_header(b"YUV4MPEG2 W128 H96 X" + b"c" * 2000 + b"\n")
