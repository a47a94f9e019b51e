"""dcvc on pipes on a real MI355X: pictures and streams through stdin, stdout and FIFOs against the SAME tool
run on regular files in the same test - the stream, the reconstruction and the logs must not differ by a byte - and the two
tools connected by a pipe, where the first decoded picture must arrive before the encoder has seen the end of its input.
96x128 clips of synthetic.synthetic_frame_yuv420, seeded synthetic weights as test_cli_gpu.py builds them. stdin is fed from a
thread in writes of 4099 bytes, so that the tool's reads end inside pictures. Every subprocess has a time limit and is
killed in a finally: a pipe run that would block fails instead of hanging."""
import json
import os
import subprocess
import threading

import numpy as np
import pytest

import wire_np as wn
from codec_util import dmc_ht_model, dmc_ld_model, dmci_model
from dcvc_amd import export_weights, stream_helper as sh, synthetic

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "dcvc_amd", "bin", "dcvc")
H, W = 96, 128
SIZE = ["-W", str(W), "-H", str(H)]
QP = ["--qp-i", "30", "--qp-p", "36", "--reset-interval", "4"]
FRAME = H * W * 3 // 2
CHUNK = 4099
LIMIT = 120


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    """models, and the file runs that several tests compare against, made once"""
    assert os.path.exists(TOOL), "dcvc_amd/bin/dcvc is built by python -m dcvc_amd.build"
    d = tmp_path_factory.mktemp("pipe")
    export_weights.write_dcvw(str(d / "i.dcvw"), "dmci", dmci_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "ld.dcvw"), "ld", dmc_ld_model(skip_thres=0.15), 0.15)
    export_weights.write_dcvw(str(d / "hts.dcvw"), "hts", dmc_ht_model("hts", skip_thres=0.15), 0.15)
    return _Work(d)


class _Work:
    def __init__(self, d):
        self.d = d
        self._clips, self._streams, self._recs = {}, {}, {}

    def models(self, kind):
        m = ["--intra", str(self.d / "i.dcvw")]
        return m if kind == "intra" else m + ["--inter", str(self.d / (kind + ".dcvw"))]

    def clip(self, n):
        """n raw 8-bit 4:2:0 pictures -> (path, bytes)"""
        if n not in self._clips:
            data = b"".join(_picture(i) for i in range(n))
            path = self.d / ("in%d.yuv" % n)
            path.write_bytes(data)
            self._clips[n] = (str(path), data)
        return self._clips[n]

    def stream(self, kind, n, extra=()):
        """the stream of the file run: encode -i in.yuv -o out.bin"""
        key = (kind, n, tuple(extra))
        if key not in self._streams:
            out = self.d / ("out%d.bin" % len(self._streams))
            _run(["encode"] + self.models(kind) + QP + SIZE + ["-i", self.clip(n)[0], "-o", str(out)] + list(extra))
            self._streams[key] = (str(out), out.read_bytes())
        return self._streams[key]

    def rec(self, kind, n):
        """the file run's decode with --ref and --json -> (rec.yuv's bytes, the log without test_time)"""
        key = (kind, n)
        if key not in self._recs:
            rec, log = self.d / ("rec%d.yuv" % len(self._recs)), self.d / ("log%d.json" % len(self._recs))
            _run(["decode"] + self.models(kind) + ["-i", self.stream(kind, n)[0], "-o", str(rec), "--ref", self.clip(n)[0], "--json", str(log)])
            self._recs[key] = (rec.read_bytes(), _numbers(log))
        return self._recs[key]


def _picture(i):
    y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
    return y.tobytes() + uv.tobytes()


def _picture_422p10(i):
    """planar 10-bit 4:2:2 samples (u16): the 4:2:0 picture with its chroma rows repeated, times 4 plus the index"""
    y, uv = synthetic.synthetic_frame_yuv420(H, W, index=i, seed=3)
    uv = np.repeat(uv, 2, axis=1)
    return np.concatenate([(p.astype(np.uint16) * 4 + (i & 3)).ravel() for p in (y, uv)])


def _numbers(path):
    log = json.loads(open(path).read())
    log.pop("test_time")
    return log


def _run(args):
    return subprocess.run([TOOL] + args, check=True, capture_output=True, text=True, timeout=LIMIT)


def _write(f, mv):
    while len(mv):
        mv = mv[f.write(mv):]


def _feed(f, data, gate=None, first=0):
    """writes of CHUNK bytes into the raw pipe f, then closes it; with a gate: `first` bytes, and the rest once the gate opens
    (if it does not, the input ends there and the caller's comparison fails)"""
    try:
        mv = memoryview(data)
        head = len(data) if gate is None else first
        for at in range(0, head, CHUNK):
            _write(f, mv[at:min(at + CHUNK, head)])
        if gate is not None and gate.wait(LIMIT):
            for at in range(head, len(data), CHUNK):
                _write(f, mv[at:at + CHUNK])
    except OSError:
        pass                               # the tool has gone: its status and stderr tell
    finally:
        try:
            f.close()
        except OSError:
            pass


def _piped(args, data):
    """the tool with `data` on stdin -> (status, stdout bytes, stderr text)"""
    proc = subprocess.Popen([TOOL] + args, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.PIPE, bufsize=0)
    stdin, proc.stdin = proc.stdin, None               # communicate() must not close what the feeder writes
    t = threading.Thread(target=_feed, args=(stdin, data), daemon=True)
    t.start()
    try:
        out, err = proc.communicate(timeout=LIMIT)
        status = proc.returncode
    finally:
        proc.kill()
        proc.wait()
        t.join(10)
    return status, out, err.decode("utf-8", "replace")


def _ok(r):
    assert r[0] == 0, r[2]
    return r


# ------------------------------------------------------------------------------------ encode from stdin to stdout
@pytest.mark.parametrize("kind,n,extra", [("intra", 3, []), ("ld", 6, []), ("hts", 11, []), ("intra", 3, ["--batch", "2"])],
                         ids=["intra", "ld", "hts-ragged", "intra-batch2"])
def test_encode_stdin_to_stdout_equals_the_file_run(work, kind, n, extra):
    want = work.stream(kind, n, extra)[1]
    status, out, err = _ok(_piped(["encode"] + work.models(kind) + QP + SIZE + ["-i", "-", "-o", "-"] + extra, work.clip(n)[1]))
    assert out == want, "stdout is not the file run's stream (and nothing else)"
    assert "encoded %d pictures" % n in err                                   # the messages went to stderr
    if extra:
        assert want == work.stream(kind, n)[1]


def _y4m(tag, pictures):
    return ("YUV4MPEG2 W%d H%d F30:1 Ip %s\n" % (W, H, tag)).encode() + b"".join(b"FRAME\n" + p for p in pictures)


@pytest.mark.parametrize("tag", ["C420jpeg", "C422p10"])
def test_y4m_on_stdin(work, tmp_path, tag):
    pics = [_picture(i) for i in range(3)] if tag == "C420jpeg" else [_picture_422p10(i).astype("<u2").tobytes() for i in range(3)]
    data = _y4m(tag, pics)
    (tmp_path / "in.y4m").write_bytes(data)
    _run(["encode"] + work.models("ld") + QP + ["-i", str(tmp_path / "in.y4m"), "-o", str(tmp_path / "out.bin")])
    want = (tmp_path / "out.bin").read_bytes()
    status, out, err = _ok(_piped(["encode"] + work.models("ld") + QP + ["-i", "-", "--in-format", "y4m", "-o", "-"], data))
    assert out == want


def test_v210_on_stdin(work, tmp_path):
    data = b"".join(wn.pack(_picture_422p10(i), wn.V210, 10, H, W).tobytes() for i in range(3))
    assert len(data) == 3 * wn.picture_bytes(wn.V210, 10, H, W)
    (tmp_path / "in.v210").write_bytes(data)
    flags = work.models("ld") + QP + SIZE + ["--src-type", "v210"]
    _run(["encode"] + flags + ["-i", str(tmp_path / "in.v210"), "-o", str(tmp_path / "out.bin")])
    status, out, err = _ok(_piped(["encode"] + flags + ["-i", "-", "-o", "-"], data))
    assert out == (tmp_path / "out.bin").read_bytes()


def test_a_truncated_y4m_pipe_keeps_the_complete_units(work):
    n = 3
    full = work.stream("intra", n)[1]
    data = _y4m("C420jpeg", [_picture(i) for i in range(n)])
    cut = data[:len(data) - FRAME // 3]                                       # the input ends inside the last picture
    status, out, err = _piped(["encode"] + work.models("intra") + QP + ["-i", "-", "--in-format", "y4m", "-o", "-"], cut)
    assert status == 2 and "ends inside a picture" in err, (status, err)
    # the parameter set and the first two I units of the file run's stream, and not a byte more
    sizes = []
    buf = full
    while buf:
        rc, _ = sh.next_unit(buf, True)
        sizes.append(rc)
        buf = buf[rc:]
    assert len(sizes) == 1 + n
    assert out == full[:sum(sizes[:n])]
    # a raw pipe that ends inside a picture: the partial picture is dropped with a warning, as size / frame_bytes drops it
    raw = work.clip(n)[1]
    status, out, err = _ok(_piped(["encode"] + work.models("intra") + QP + SIZE + ["-i", "-", "-o", "-"], raw[:len(raw) - FRAME // 3]))
    assert out == full[:sum(sizes[:n])] and "warning" in err and "encoded 2 pictures" in err


# ------------------------------------------------------------------------------------ decode from stdin to stdout
def test_decode_stdin_to_stdout(work, tmp_path):
    stream = work.stream("intra", 3)[1]
    want_rec, _ = work.rec("intra", 3)
    status, out, err = _ok(_piped(["decode"] + work.models("intra") + ["-i", "-", "-o", "-"], stream))
    assert out == want_rec and "decoded 3 pictures" in err


def test_decode_stdin_with_ref_and_log(work, tmp_path):
    stream = work.stream("ld", 6)[1]
    want_rec, want_log = work.rec("ld", 6)
    status, out, err = _ok(_piped(["decode"] + work.models("ld") + ["-i", "-", "-o", "-", "--ref", work.clip(6)[0], "--json",
                                                                    str(tmp_path / "log.json")], stream))
    assert out == want_rec
    assert _numbers(tmp_path / "log.json") == want_log


def test_decode_hts_from_stdin_trims_the_padding_with_ref(work, tmp_path):
    stream = work.stream("hts", 11)[1]
    want_rec, want_log = work.rec("hts", 11)
    assert len(want_rec) == 11 * FRAME
    status, out, err = _ok(_piped(["decode"] + work.models("hts") + ["-i", "-", "-o", "-", "--ref", work.clip(11)[0], "--json",
                                                                     str(tmp_path / "log.json")], stream))
    assert out == want_rec and "decoded 11 pictures" in err
    assert _numbers(tmp_path / "log.json") == want_log


def test_decode_out_format_y4m(work, tmp_path):
    path, stream = work.stream("intra", 3)
    _run(["decode"] + work.models("intra") + ["-i", path, "-o", str(tmp_path / "rec.y4m")])
    want = (tmp_path / "rec.y4m").read_bytes()
    assert want.startswith(b"YUV4MPEG2 ") and want.count(b"FRAME\n") >= 3
    status, out, err = _ok(_piped(["decode"] + work.models("intra") + ["-i", "-", "-o", "-", "--out-format", "y4m"], stream))
    assert out == want


def test_decode_ref_through_a_fifo(work, tmp_path):
    path, _ = work.stream("ld", 6)
    _, want_log = work.rec("ld", 6)
    fifo = str(tmp_path / "ref.fifo")
    os.mkfifo(fifo)
    proc = subprocess.Popen([TOOL, "decode"] + work.models("ld") + ["-i", path, "--ref", fifo, "--json", str(tmp_path / "log.json")],
                            stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE)

    def writer():
        # opening a FIFO waits for its reader: the tool, or - should it fail before it opens --ref - the finally below
        _feed(open(fifo, "wb", buffering=0), work.clip(6)[1])

    t = threading.Thread(target=writer, daemon=True)
    t.start()
    try:
        out, err = proc.communicate(timeout=LIMIT)
        assert proc.returncode == 0, err.decode()
    finally:
        proc.kill()
        proc.wait()
        if t.is_alive():                   # release a writer that still waits in open()
            try:
                os.close(os.open(fifo, os.O_RDONLY | os.O_NONBLOCK))
            except OSError:
                pass
        t.join(10)
    assert _numbers(tmp_path / "log.json") == want_log


# ------------------------------------------------------------------------------------ read-ahead
@pytest.mark.parametrize("extra", [[], ["--scale", "64x48"]], ids=["ld", "ld-scale"])
def test_read_ahead_does_not_change_the_stream(work, extra):
    want = work.stream("ld", 6, extra)[1]
    for ra in ("0", "1", "4"):
        status, out, err = _ok(_piped(["encode"] + work.models("ld") + QP + SIZE + ["-i", "-", "-o", "-", "--read-ahead", ra] + extra,
                                      work.clip(6)[1]))
        assert out == want, "--read-ahead " + ra


# ------------------------------------------------------------------------------------ rate control and scene cuts
@pytest.mark.parametrize("flags,log", [(["--target-bpp", "0.5"], "--rc-log"), (["--scene-cut", "5"], "--scene-log")], ids=["target-bpp", "scene-cut"])
def test_rate_control_and_scene_cuts_on_stdin(work, tmp_path, flags, log):
    qp = ["--qp-i", "30", "--reset-interval", "4"]                            # --qp-p is refused with --target-bpp
    base = ["encode"] + work.models("ld") + qp + SIZE + flags
    _run(base + ["-i", work.clip(6)[0], "-o", str(tmp_path / "out.bin"), log, str(tmp_path / "file.json")])
    status, out, err = _ok(_piped(base + ["-i", "-", "-o", "-", log, str(tmp_path / "pipe.json")], work.clip(6)[1]))
    assert out == (tmp_path / "out.bin").read_bytes()
    assert json.loads((tmp_path / "pipe.json").read_text()) == json.loads((tmp_path / "file.json").read_text())
    assert ("rate control:" if log == "--rc-log" else "scene cut:") in err


# ------------------------------------------------------------------------------------ the live chain
def _check_latency(log, stream_bytes, pictures):
    units = log["units"]
    assert [u["pictures"] for u in units] == pictures and log["pictures"] == sum(pictures)
    assert [u["first_picture"] for u in units] == [sum(pictures[:i]) for i in range(len(pictures))]
    assert sum(u["bytes"] for u in units) == stream_bytes == log["bytes"]
    for a, b in zip(units, units[1:]):
        assert b["read_ms"] >= a["read_ms"] and b["out_ms"] >= a["out_ms"]
    assert all(u["out_ms"] >= u["read_ms"] >= 0 for u in units)


@pytest.mark.parametrize("kind,n", [("intra", 5), ("ld", 6)])
def test_live_chain(work, tmp_path, kind, n):
    """encode | decode, both running: the feeder holds the clip's end back until the decoder has delivered a whole picture, so the
    run ends only if neither side waits for the end of its input"""
    data = work.clip(n)[1]
    want_stream = work.stream(kind, n)[1]
    want_rec, _ = work.rec(kind, n)
    lat = tmp_path / "lat.json"
    got = bytearray()
    first_picture = threading.Event()
    enc = dec = None
    threads = []
    with open(tmp_path / "enc.err", "wb") as enc_err, open(tmp_path / "dec.err", "wb") as dec_err:
        try:
            enc = subprocess.Popen([TOOL, "encode"] + work.models(kind) + QP + SIZE + ["-i", "-", "-o", "-", "--read-ahead", "2", "--latency-log",
                                                                                      str(lat)], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                   stderr=enc_err, bufsize=0)
            dec = subprocess.Popen([TOOL, "decode"] + work.models(kind) + ["-i", "-", "-o", "-"], stdin=enc.stdout, stdout=subprocess.PIPE,
                                   stderr=dec_err, bufsize=0)
            enc.stdout.close()             # the decoder holds the read end now

            def collect():
                while True:
                    piece = dec.stdout.read(65536)
                    if not piece:
                        return
                    got.extend(piece)
                    if len(got) >= FRAME:
                        first_picture.set()

            threads = [threading.Thread(target=collect, daemon=True),
                       threading.Thread(target=_feed, args=(enc.stdin, data, first_picture, 3 * FRAME), daemon=True)]
            for t in threads:
                t.start()
            assert first_picture.wait(LIMIT), "no decoded picture while the encoder's input was still open"
            assert enc.wait(LIMIT) == 0 and dec.wait(LIMIT) == 0
            threads[0].join(LIMIT)
        finally:
            first_picture.set()
            for p in (enc, dec):
                if p is not None:
                    p.kill()
                    p.wait()
            for t in threads:
                t.join(10)
    assert bytes(got) == want_rec, (tmp_path / "dec.err").read_text()
    log = json.loads(lat.read_text())
    _check_latency(log, len(want_stream), [1] * n)
    # the first unit had left the encoder before the clip's last picture reached it
    assert log["units"][0]["out_ms"] < log["units"][-1]["read_ms"]


# ------------------------------------------------------------------------------------ regular files
def test_flush_units_on_a_regular_file_and_the_latency_log(work, tmp_path):
    want = work.stream("hts", 11)[1]
    base = ["encode"] + work.models("hts") + QP + SIZE + ["-i", work.clip(11)[0]]
    r = _run(base + ["-o", str(tmp_path / "flushed.bin"), "--flush-units", "1", "--latency-log", str(tmp_path / "flushed.json")])
    assert (tmp_path / "flushed.bin").read_bytes() == want and "encoded 11 pictures" in r.stdout
    _check_latency(json.loads((tmp_path / "flushed.json").read_text()), len(want), [1, 8, 2])
    # without the flag the file is written once at the end: every unit's out_ms is that write
    _run(base + ["-o", str(tmp_path / "plain.bin"), "--latency-log", str(tmp_path / "plain.json")])
    log = json.loads((tmp_path / "plain.json").read_text())
    assert (tmp_path / "plain.bin").read_bytes() == want
    _check_latency(log, len(want), [1, 8, 2])
    assert log["units"][0]["out_ms"] >= log["units"][-1]["read_ms"] and [u["type"] for u in log["units"]] == ["I", "P", "P"]
