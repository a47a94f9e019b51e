"""The feed-style container parser (dcvc_stream_next_unit, include/dcvc_amd_stream.h) against the whole-buffer
readers beside it: the same units field by field, every strict prefix of every unit answered with a `need` inside
(prefix, unit length], feeding by single bytes and by reads of exactly `need`, the malformed headers with the readers'
status and message, and the Python mirror stream_helper.next_unit / iter_units. CPU only: host code of the library."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

from dcvc_amd import _lib, stream_helper as sh
from test_stream_native import _python_bytes, _sequence

ci, cz = ctypes.c_int, ctypes.c_size_t
vp = ctypes.c_void_p


def _own_sequence():
    """every payload length at which the length field changes its size, and two parameter sets"""
    rng = np.random.default_rng(11)
    units = [("sps", 0, 1080, 1920)]
    for i, n in enumerate([0, 1, 127, 128, 16383, 16384, 70000]):
        if i == 3:
            units.append(("sps", 1, 96, 128))
        units.append(("ip", i % 3 == 0, i % 2, int(rng.integers(0, 256)), int(rng.integers(0, 128)), int(rng.integers(0, 2)),
                      rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    return units


@pytest.fixture(scope="module")
def nat():
    f = _lib.fn
    return dict(
        next_unit=f("dcvc_stream_next_unit", ctypes.c_int64, [vp, cz, ci, ctypes.POINTER(sh._Unit)]),
        read_header=f("dcvc_stream_read_header", ci, [vp, cz, ctypes.POINTER(ci), ctypes.POINTER(ci)]),
        read_sps=f("dcvc_stream_read_sps_remaining", ci, [vp, cz, ctypes.POINTER(ci), ctypes.POINTER(ci)]),
        read_ip=f("dcvc_stream_read_ip_remaining", ctypes.c_int64,
                  [vp, cz, ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(vp), ctypes.POINTER(cz)]),
    )


@pytest.fixture(scope="module", params=["own", "golden"])
def stream(request, golden_dir):
    """(bytes, ctypes buffer over them, units as written)"""
    units = _own_sequence() if request.param == "own" else _sequence()
    data = _python_bytes(units)
    if request.param == "golden":
        with open(os.path.join(golden_dir, "stream_golden.json")) as f:
            want = json.load(f)
        assert len(data) == want["bytes"] and hashlib.sha256(data).hexdigest() == want["sha256"]
    return data, (ctypes.c_uint8 * len(data)).from_buffer_copy(data), [tuple(u) for u in units]


def _unit_tuple(u, base, data):
    """a filled dcvc_stream_unit at offset `base` of `data` -> the tuple _sequence() describes the unit with"""
    if u.nal_type == 0:
        return ("sps", u.sps_id, u.height, u.width)
    assert u.payload_offset + u.payload_bytes == u.unit_bytes          # the payload ends the unit
    return ("ip", u.nal_type == 1, u.sps_id, u.qp, u.ec_part, u.reset, data[base + u.payload_offset:base + u.unit_bytes])


def _readers_units(nat, data, buf):
    """the units as read_header / read_sps_remaining / read_ip_remaining give them, with their lengths"""
    addr, pos, seen = ctypes.addressof(buf), 0, []
    while pos < len(data):
        nal, sid = ci(), ci()
        assert nat["read_header"](addr + pos, len(data) - pos, ctypes.byref(nal), ctypes.byref(sid)) == 1
        if nal.value == 0:
            h, w = ci(), ci()
            k = nat["read_sps"](addr + pos + 1, len(data) - pos - 1, ctypes.byref(h), ctypes.byref(w))
            seen.append((("sps", sid.value, h.value, w.value), 1 + k))
        else:
            qp, ec, rs, n, pl = ci(), ci(), ci(), cz(), vp()
            k = nat["read_ip"](addr + pos + 1, len(data) - pos - 1, ctypes.byref(qp), ctypes.byref(ec), ctypes.byref(rs),
                               ctypes.byref(pl), ctypes.byref(n))
            seen.append((("ip", nal.value == 1, sid.value, qp.value, ec.value, rs.value, ctypes.string_at(pl.value, n.value)), 1 + k))
        assert k > 0
        pos += 1 + k
    return seen


def test_whole_buffer_gives_the_readers_units(nat, stream):
    data, buf, units = stream
    want = _readers_units(nat, data, buf)
    assert [w[0] for w in want] == units
    addr, pos, u = ctypes.addressof(buf), 0, sh._Unit()
    for fields, length in want:
        rc = nat["next_unit"](addr + pos, len(data) - pos, 1, ctypes.byref(u))
        assert rc == length == u.unit_bytes and u.need == 0
        assert _unit_tuple(u, pos, data) == fields
        pos += rc
    assert pos == len(data)                                                  # the consumed bytes add up to the length
    assert nat["next_unit"](addr + pos, 0, 1, ctypes.byref(u)) == 0 and u.need == 0      # the clean end


def test_every_strict_prefix_of_every_unit(nat, stream):
    data, buf, _ = stream
    addr, pos, u = ctypes.addressof(buf), 0, sh._Unit()
    fn = nat["next_unit"]
    for _, length in _readers_units(nat, data, buf):
        for k in range(length):
            u.unit_bytes = 77                                                # nothing is consumed, nothing reported as a unit
            assert fn(addr + pos, k, 0, ctypes.byref(u)) == 0 and k < u.need <= length and u.unit_bytes == 0, (pos, k, u.need)
            rc = fn(addr + pos, k, 1, ctypes.byref(u))
            if k == 0:
                assert rc == 0 and u.need == 0
            else:
                assert rc == -2, (pos, k, rc)
        pos += length
    assert "truncated" in _lib.lib().dcvc_last_error().decode()


@pytest.mark.parametrize("step", ["one byte", "need"])
def test_feeding_reproduces_the_unit_list(nat, stream, step):
    data, buf, units = stream
    addr, u = ctypes.addressof(buf), sh._Unit()
    start, have, seen = 0, 0, []                 # the unit being fed starts at `start`; `have` bytes of the stream were fed
    while True:
        at_eof = have == len(data)
        rc = nat["next_unit"](addr + start, have - start, 1 if at_eof else 0, ctypes.byref(u))
        assert rc >= 0
        if rc > 0:
            seen.append(_unit_tuple(u, start, data))
            start += rc
            assert start <= have
            continue
        if u.need == 0:
            break
        assert u.need > have - start
        have = have + 1 if step == "one byte" else start + u.need
        assert have <= len(data)                 # `need` never asks for more than the unit holds
        if step == "need":
            assert have - start <= len(data) - start
    assert seen == units and start == len(data)


def test_malformed_headers_as_the_readers_refuse_them(nat):
    u, nal, sid = sh._Unit(), ci(), ci()
    err = lambda: _lib.lib().dcvc_last_error().decode()
    for first in range(0x30, 0x100, 0x0D):                                  # unit types 3..15
        head = bytes([first, 1, 2, 3, 4, 5])
        for n in (1, len(head)):
            assert nat["read_header"](head, n, ctypes.byref(nal), ctypes.byref(sid)) == -3
            want = err()
            for at_eof in (0, 1):
                assert nat["next_unit"](head, n, at_eof, ctypes.byref(u)) == -3
                assert err() == want and "unknown unit type" in want
    # a length field that announces more than the buffer holds is truncation (-2), as read_ip_remaining says
    short = bytes([0x10, 32, 3, 10, 1, 2, 3])
    qp, ec, rs, n, pl = ci(), ci(), ci(), cz(), vp()
    assert nat["read_ip"](short[1:], len(short) - 1, ctypes.byref(qp), ctypes.byref(ec), ctypes.byref(rs), ctypes.byref(pl),
                          ctypes.byref(n)) == -2
    want = err()
    assert nat["next_unit"](short, len(short), 1, ctypes.byref(u)) == -2 and err() == want
    assert nat["next_unit"](short, len(short), 0, ctypes.byref(u)) == 0 and u.need == 14


class _Dribble:
    """a source that has read(n) and nothing else, and hands out at most 7 bytes a call"""

    def __init__(self, data):
        self._data, self._pos, self.calls = data, 0, 0

    def read(self, n):
        k = min(n, 7)
        out = self._data[self._pos:self._pos + k]
        self._pos += len(out)
        self.calls += 1
        return out


def _as_tuple(d):
    if d["nal_type"] == sh.NalType.NAL_SPS:
        return ("sps", d["sps_id"], d["height"], d["width"])
    return ("ip", d["nal_type"] == sh.NalType.NAL_I, d["sps_id"], d["qp"], d["ec_part"], d["reset"], d["payload"])


def test_python_mirror_next_unit_and_iter_units(stream):
    data, _, units = stream
    rc, first = sh.next_unit(data, True)
    assert rc == 5 and _as_tuple(first) == units[0]              # header, two 2-byte sides (1080 x 1920)
    assert sh.next_unit(data[:1], False) == (0, {"need": 3})      # ... each at least one byte, as far as one byte tells
    assert sh.next_unit(data[:2], False) == (0, {"need": 4})
    assert sh.next_unit(b"", True) == (0, {"need": 0})
    with pytest.raises(_lib.DcvcError, match="truncated"):
        sh.next_unit(data[:2], True)
    with pytest.raises(_lib.DcvcError, match="unknown unit type"):
        sh.next_unit(b"\x70", False)
    src = _Dribble(data)
    assert [_as_tuple(d) for d in sh.iter_units(src)] == units
    assert not hasattr(src, "seek") and not hasattr(src, "tell")
    with pytest.raises(_lib.DcvcError, match="truncated"):
        list(sh.iter_units(_Dribble(data[:-1])))
