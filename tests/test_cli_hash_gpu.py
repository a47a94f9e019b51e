"""dcvc --hash-log / --verify-hash on a real MI355X (-m gpu), DESIGN.md 19: the manifest's CRCs are zlib.crc32 of the bytes -o
writes - per plane, per picture and over the sequence - for every output type, with and without -o, for LD and HT-S streams;
--verify-hash accepts its own manifest, reports the first mismatch with status 3 and refuses another size with status 2;
encode --hash-log writes the decoder's manifest byte for byte; without the flags nothing changes."""
import os
import subprocess
import zlib

import pytest

from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, picture_hash as ph, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W, N = 48, 64, 3


def _run(args, check=True):
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    return subprocess.run([TOOL] + [str(a) for a in args], check=check, capture_output=True, text=True, timeout=600)


def _write_yuv(path, h, w, n):
    with open(path, "wb") as f:
        for i in range(n):
            y, uv = synthetic.synthetic_frame_yuv420(h, w, index=i, seed=3)
            f.write(y.tobytes() + uv.tobytes())


def _manifest_of(data, src_type, depth, w, h):
    """the manifest of a raw -o file, from zlib"""
    lens = ph.plane_bytes(src_type, depth, w, h)
    fb = sum(lens)
    assert len(data) % fb == 0
    pictures = []
    for at in range(0, len(data), fb):
        pic, planes, o = data[at:at + fb], [], 0
        for n in lens:
            planes.append(zlib.crc32(pic[o:o + n]))
            o += n
        pictures.append((zlib.crc32(pic), planes))
    m = ph.Manifest(src_type, depth, w, h, pictures, zlib.crc32(data), len(data))
    return ph.format_manifest(m)


class Clip:
    """an all-intra stream of N 64x48 pictures, its reconstruction and its manifest, shared by the tests"""

    def __init__(self, d):
        self.d = d
        export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
        self.intra = ["--intra", d / "i.dcvw"]
        _write_yuv(str(d / "in.yuv"), H, W, N)
        self.encode = ["encode"] + self.intra + ["-i", d / "in.yuv", "-W", W, "-H", H, "--qp-i", 30]
        _run(self.encode + ["-o", d / "a.bin"])
        self.decode = ["decode"] + self.intra + ["-i", d / "a.bin"]
        _run(self.decode + ["-o", d / "rec.yuv", "--hash-log", d / "m.txt"])
        self.rec = (d / "rec.yuv").read_bytes()
        self.manifest = (d / "m.txt").read_bytes()


@pytest.fixture(scope="module")
def clip(tmp_path_factory):
    return Clip(tmp_path_factory.mktemp("hash_clip"))


def test_intra_yuv420_manifest_is_zlibs_and_needs_no_output_file(clip, tmp_path):
    assert len(clip.rec) == N * H * W * 3 // 2
    want = _manifest_of(clip.rec, "yuv420", 8, W, H)
    assert clip.manifest.decode() == want
    lines = want.split("\n")
    assert lines[0] == "# dcvc-hash 1 crc32 yuv420 8 %d %d" % (W, H) and len(lines) == N + 3
    assert lines[N + 1] == "sequence %08x %d" % (zlib.crc32(clip.rec), len(clip.rec))
    m = ph.read_manifest(str(clip.d / "m.txt"))
    assert len(m.pictures) == N and len({c for c, _ in m.pictures}) == N
    # without -o (and with --ref, which changes nothing): the same manifest, byte for byte
    _run(clip.decode + ["--hash-log", tmp_path / "m2.txt"])
    _run(clip.decode + ["--hash-log", tmp_path / "m3.txt", "--ref", clip.d / "in.yuv", "--json", tmp_path / "log.json"])
    assert (tmp_path / "m2.txt").read_bytes() == clip.manifest and (tmp_path / "m3.txt").read_bytes() == clip.manifest


OUTPUT_TYPES = [
    ("yuv420_10bit", ["--bit-depth", 10], "yuv420", 10),
    ("nv12", ["--src-type", "nv12"], "nv12", 8),
    ("p010", ["--src-type", "p010"], "nv12", 10),
    ("yuv444", ["--src-type", "yuv444"], "yuv444", 8),
    ("yuv422_12bit", ["--src-type", "yuv422", "--bit-depth", 12], "yuv422", 12),
    ("rgb24", ["--src-type", "rgb24"], "rgb24", 8),
]


@pytest.mark.parametrize("name,flags,src_type,depth", OUTPUT_TYPES, ids=[t[0] for t in OUTPUT_TYPES])
def test_other_output_types(clip, tmp_path, name, flags, src_type, depth):
    # (the stream does not carry the type: the all-intra clip is decoded to every one of them)
    _run(clip.decode + flags + ["-o", tmp_path / "rec.raw", "--hash-log", tmp_path / "m.txt"])
    want = _manifest_of((tmp_path / "rec.raw").read_bytes(), src_type, depth, W, H)
    assert (tmp_path / "m.txt").read_text() == want
    _run(clip.decode + flags + ["--hash-log", tmp_path / "m2.txt"])                       # nothing leaves the device
    assert (tmp_path / "m2.txt").read_text() == want


def test_png_hashes_the_packed_rgb_and_y4m_no_frame_lines(clip, tmp_path):
    _run(clip.decode + ["--src-type", "rgb24", "-o", tmp_path / "rec.rgb"])
    _run(clip.decode + ["--src-type", "png", "-o", tmp_path / "pngs", "--hash-log", tmp_path / "m.txt"])
    assert sorted(os.listdir(tmp_path / "pngs")) == ["im%05d.png" % (i + 1) for i in range(N)]
    assert (tmp_path / "m.txt").read_text() == _manifest_of((tmp_path / "rec.rgb").read_bytes(), "png", 8, W, H)
    _run(clip.decode + ["-o", tmp_path / "rec.y4m", "--hash-log", tmp_path / "my.txt"])
    assert (tmp_path / "rec.y4m").read_bytes().count(b"FRAME\n") == N
    assert (tmp_path / "my.txt").read_bytes() == clip.manifest


def test_out_size_hashes_the_resampled_picture(clip, tmp_path):
    _run(clip.decode + ["--out-size", "96x80", "-o", tmp_path / "rec.yuv", "--hash-log", tmp_path / "m.txt"])
    data = (tmp_path / "rec.yuv").read_bytes()
    assert len(data) == N * 96 * 80 * 3 // 2
    assert (tmp_path / "m.txt").read_text() == _manifest_of(data, "yuv420", 8, 96, 80)
    _run(clip.decode + ["--out-size", "96x80", "--bit-depth", 10, "--hash-log", tmp_path / "m10.txt", "-o", tmp_path / "rec10.yuv"])
    assert (tmp_path / "m10.txt").read_text() == _manifest_of((tmp_path / "rec10.yuv").read_bytes(), "yuv420", 10, 96, 80)
    _run(clip.decode + ["--out-size", "96x80", "--hash-log", tmp_path / "m2.txt"])
    assert (tmp_path / "m2.txt").read_bytes() == (tmp_path / "m.txt").read_bytes()


def _inter(tmp_path, kind, n, reset_interval):
    model = dmc_ld_model(skip_thres=0.15) if kind == "ld" else dmc_ht_model(kind, skip_thres=0.15)
    export_weights.write_dcvw(str(tmp_path / "p.dcvw"), kind, model, 0.15)
    _write_yuv(str(tmp_path / "in.yuv"), H, W, n)
    return ["--inter", tmp_path / "p.dcvw"]


def test_ld_with_a_reset(clip, tmp_path):
    n = 6
    inter = _inter(tmp_path, "ld", n, 4)
    _run(["encode"] + clip.intra + inter + ["-i", tmp_path / "in.yuv", "-W", W, "-H", H, "--qp-i", 30, "--qp-p", 36, "--reset-interval", 4,
                                            "-o", tmp_path / "ld.bin"])
    dec = ["decode"] + clip.intra + inter + ["-i", tmp_path / "ld.bin"]
    _run(dec + ["-o", tmp_path / "rec.yuv", "--hash-log", tmp_path / "m.txt"])
    data = (tmp_path / "rec.yuv").read_bytes()
    assert len(data) == n * H * W * 3 // 2
    assert (tmp_path / "m.txt").read_text() == _manifest_of(data, "yuv420", 8, W, H)
    r = _run(dec + ["--verify-hash", tmp_path / "m.txt"])
    assert "verified %d pictures" % n in r.stdout


def test_hts_ragged_last_chunk_holds_exactly_the_written_pictures(clip, tmp_path):
    n = 11                                                           # 1 + 8 + 2: six padding pictures in the last chunk
    inter = _inter(tmp_path, "hts", n, 0)
    _run(["encode"] + clip.intra + inter + ["-i", tmp_path / "in.yuv", "-W", W, "-H", H, "--qp-i", 30, "--qp-p", 36, "-o", tmp_path / "ht.bin"])
    dec = ["decode"] + clip.intra + inter + ["-i", tmp_path / "ht.bin"]
    _run(dec + ["-n", n, "-o", tmp_path / "rec.yuv", "--hash-log", tmp_path / "m.txt"])
    data = (tmp_path / "rec.yuv").read_bytes()
    assert len(data) == n * H * W * 3 // 2
    want = _manifest_of(data, "yuv420", 8, W, H)
    assert (tmp_path / "m.txt").read_text() == want and len(want.split("\n")) == n + 3
    # the source's length trims the padding pictures too, without -o; and a shorter -n gives a prefix of the manifest
    _run(dec + ["--ref", tmp_path / "in.yuv", "--hash-log", tmp_path / "m2.txt"])
    assert (tmp_path / "m2.txt").read_text() == want
    _run(dec + ["-n", 4, "--hash-log", tmp_path / "m4.txt"])
    assert (tmp_path / "m4.txt").read_text() == _manifest_of(data[:4 * H * W * 3 // 2], "yuv420", 8, W, H)


def test_verify_hash_accepts_its_own_manifest(clip, tmp_path):
    r = _run(clip.decode + ["--verify-hash", clip.d / "m.txt"], check=False)
    assert r.returncode == 0 and "verified %d pictures" % N in r.stdout, r.stderr
    # together with -o and --hash-log: both are written as without the flag
    r = _run(clip.decode + ["--verify-hash", clip.d / "m.txt", "-o", tmp_path / "rec.yuv", "--hash-log", tmp_path / "m.txt"], check=False)
    assert r.returncode == 0 and (tmp_path / "rec.yuv").read_bytes() == clip.rec and (tmp_path / "m.txt").read_bytes() == clip.manifest


def _flip_hex_digit(text, line, token):
    lines = text.split("\n")
    tok = lines[line].split(" ")
    tok[token] = tok[token][:3] + ("0" if tok[token][3] != "0" else "f") + tok[token][4:]
    lines[line] = " ".join(tok)
    return "\n".join(lines)


@pytest.mark.parametrize("k,token,names", [(1, 3, "plane 1 (U)"), (2, 1, "whole picture"), (0, 2, "plane 0 (Y)")],
                         ids=["picture_1_U", "picture_2_whole", "picture_0_Y"])
def test_verify_hash_rejects_a_changed_digit(clip, tmp_path, k, token, names):
    good = clip.manifest.decode()
    (tmp_path / "bad.txt").write_text(_flip_hex_digit(good, 1 + k, token))
    r = _run(clip.decode + ["--verify-hash", tmp_path / "bad.txt"], check=False)
    assert r.returncode == 3, (r.returncode, r.stderr)
    assert "picture %d, %s" % (k, names) in r.stderr and "expected" in r.stderr and "got" in r.stderr, r.stderr
    want_tok = good.split("\n")[1 + k].split(" ")[token]
    assert "got " + want_tok in r.stderr                      # what was decoded is the unchanged manifest's value


def test_verify_hash_rejects_another_number_of_pictures(clip, tmp_path):
    m = ph.read_manifest(str(clip.d / "m.txt"))
    # one picture line removed (a consistent manifest of the first N - 1 pictures): one more is decoded than it holds
    ph.write_manifest(str(tmp_path / "short.txt"), ph.Manifest(m.src_type, m.bit_depth, m.width, m.height, m.pictures[:-1]))
    r = _run(clip.decode + ["--verify-hash", tmp_path / "short.txt"], check=False)
    assert r.returncode == 3 and "picture %d was decoded" % (N - 1) in r.stderr and "holds %d pictures" % (N - 1) in r.stderr, r.stderr
    # the line removed and nothing else touched: the same status
    lines = clip.manifest.decode().split("\n")
    (tmp_path / "cut.txt").write_text("\n".join(lines[:N] + lines[N + 1:]))
    r = _run(clip.decode + ["--verify-hash", tmp_path / "cut.txt"], check=False)
    assert r.returncode == 3, (r.returncode, r.stderr)
    # fewer pictures decoded than the manifest holds
    r = _run(clip.decode + ["-n", N - 1, "--verify-hash", clip.d / "m.txt"], check=False)
    assert r.returncode == 3 and "%d pictures were decoded" % (N - 1) in r.stderr, r.stderr


def test_verify_hash_refuses_a_manifest_of_another_run(clip, tmp_path):
    good = clip.manifest.decode()
    cases = [(good.replace(" %d %d\n" % (W, H), " %d %d\n" % (W + 2, H), 1), [], "%dx%d pictures" % (W + 2, H)),
             (good.replace("yuv420 8", "yuv420 10", 1), [], "of 10 bits"),
             (good.replace("yuv420 8", "yuv444 8", 1), [], "yuv444"),
             (good, ["--out-size", "96x80"], "96x80")]
    for text, flags, says in cases:
        (tmp_path / "other.txt").write_text(text)
        r = _run(clip.decode + flags + ["--verify-hash", tmp_path / "other.txt", "-o", tmp_path / "rec.yuv"], check=False)
        assert r.returncode == 2 and "--verify-hash" in r.stderr and says in r.stderr, (says, r.stderr)
        assert not (tmp_path / "rec.yuv").exists() or (tmp_path / "rec.yuv").stat().st_size == 0      # no picture was decoded


@pytest.mark.parametrize("batch", [1, 3])
def test_encode_hash_log_is_the_decoders_manifest(clip, tmp_path, batch):
    _run(clip.encode + ["--batch", batch, "-o", tmp_path / "b.bin", "--hash-log", tmp_path / "enc.txt"])
    assert (tmp_path / "b.bin").read_bytes() == (clip.d / "a.bin").read_bytes()          # the flag does not touch the stream
    assert (tmp_path / "enc.txt").read_bytes() == clip.manifest


@pytest.mark.parametrize("batch", [1, 3])
def test_encode_hash_log_with_scale(clip, tmp_path, batch):
    _write_yuv(str(tmp_path / "big.yuv"), 2 * H, 2 * W, N)
    enc = ["encode"] + clip.intra + ["-i", tmp_path / "big.yuv", "-W", 2 * W, "-H", 2 * H, "--qp-i", 30, "--scale", "%dx%d" % (W, H),
                                     "--batch", batch]
    _run(enc + ["-o", tmp_path / "s.bin", "--hash-log", tmp_path / "enc.txt"])
    _run(["decode"] + clip.intra + ["-i", tmp_path / "s.bin", "--batch", batch, "-o", tmp_path / "rec.yuv", "--hash-log", tmp_path / "dec.txt"])
    assert (tmp_path / "enc.txt").read_bytes() == (tmp_path / "dec.txt").read_bytes()
    assert (tmp_path / "dec.txt").read_text() == _manifest_of((tmp_path / "rec.yuv").read_bytes(), "yuv420", 8, W, H)


def test_encode_hash_log_at_10_bits_nv12(clip, tmp_path):
    # the source's type and depth: P010 in, the decoder's P010 manifest out
    import numpy as np
    rng = np.random.default_rng(8)
    (tmp_path / "in.p010").write_bytes((rng.integers(0, 1024, N * H * W * 3 // 2, dtype=np.uint16) << 6).astype("<u2").tobytes())
    kind = ["--src-type", "p010"]
    _run(["encode"] + clip.intra + kind + ["-i", tmp_path / "in.p010", "-W", W, "-H", H, "--qp-i", 30, "-o", tmp_path / "p.bin",
                                           "--hash-log", tmp_path / "enc.txt"])
    _run(["decode"] + clip.intra + kind + ["-i", tmp_path / "p.bin", "-o", tmp_path / "rec.p010", "--hash-log", tmp_path / "dec.txt"])
    assert (tmp_path / "enc.txt").read_bytes() == (tmp_path / "dec.txt").read_bytes()
    assert (tmp_path / "dec.txt").read_text() == _manifest_of((tmp_path / "rec.p010").read_bytes(), "nv12", 10, W, H)


def test_flags_off_changes_nothing(clip, tmp_path):
    # the stream and rec.yuv of runs without the flags equal the ones with them (the clip's rec.yuv came with --hash-log)
    _run(clip.decode + ["-o", tmp_path / "rec.yuv"])
    assert (tmp_path / "rec.yuv").read_bytes() == clip.rec
    _run(clip.encode + ["-o", tmp_path / "b.bin", "--hash-log", tmp_path / "enc.txt"])
    assert (tmp_path / "b.bin").read_bytes() == (clip.d / "a.bin").read_bytes()
    assert sorted(os.listdir(tmp_path)) == ["b.bin", "enc.txt", "rec.yuv"]
