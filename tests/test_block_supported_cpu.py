"""The set of shapes the fused block kernels answer for, frozen (no GPU: the three queries are host code).

dcvc_dcb_nsplit_fin_supported, dcvc_dcb_nsplit_dw_supported and dcvc_dcb_pair_supported decide what DcbW::load packs and what
DcbW::forward fuses. A shape that drops out of one of them is not an error anywhere: the codecs fall back to the launch
sequence, which is bit-identical, so every parity test stays green while a codec gets slower. The lists below are literal.

The A/B switches (DCVC_NSPLIT_FIN, DCVC_NSPLIT_DW, DCVC_NSPLIT_PX, DCVC_PAIR, ...) are read once per process and change the
answers, so the queries run in ONE fresh child process with every DCVC_* switch taken out of its environment: the test
never skips, whatever the caller has exported."""
import itertools
import json
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_block_pack_gpu as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (128, 192, 256, 384, 448, 512, 768)
SHAPES = [(256, 256), (384, 384), (512, 512), (768, 768), (512, 256), (256, 128), (384, 192), (192, 192)]
FINS = [(256, 128, 128), (256, 128, 192), (256, 128, 256), (256, 256, 192), (512, 512, 256), (512, 512, 512), (768, 768, 768),
        (384, 192, 384)]
# depthwise conv inside the launch: (C, CI) -> answer at each of DW_PIXELS ((384, 192): 32-pixel workgroups only, (384, 384): none)
DW_PIXELS = (0, 64, 12799, 12800, 32640)
DW = {(256, 128): (0, 1, 1, 1, 1), (384, 192): (0, 1, 1, 0, 0), (384, 384): (0, 0, 0, 0, 0)}
ADAPTORS = [(448, 256, 128), (512, 256, 128), (192, 256, 128), (128, 256, 256), (512, 256, 256), (192, 384, 384),
            (384, 192, 192), (256, 512, 512), (512, 512, 512), (192, 512, 512), (192, 512, 256)]

CHILD = """
import ctypes, itertools, json, sys
sys.path.insert(0, %r)
from dcvc_amd import _lib
i = ctypes.c_int
W, PX = %r, %r
fin = _lib.fn("dcvc_dcb_nsplit_fin_supported", i, [i, i, i])
dw = _lib.fn("dcvc_dcb_nsplit_dw_supported", i, [i, i, i])
pair = _lib.fn("dcvc_dcb_pair_supported", i, [i, i, i])
print(json.dumps({"fin": [fin(*t) for t in itertools.product(W, repeat=3)],
                  "pair": [pair(*t) for t in itertools.product(W, repeat=3)],
                  "dw": [[dw(c, ci, p) for p in PX] for c, ci in itertools.product(W, repeat=2)]}))
"""


@pytest.fixture(scope="module")
def answers():
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCVC_") or k == "DCVC_LIB"}
    r = subprocess.run([sys.executable, "-s", "-c", CHILD % (ROOT, WIDTHS, DW_PIXELS)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_closing_convs(answers):
    assert len(SHAPES) == 8 and {(c, ci) for c, ci, _ in FINS} <= set(SHAPES)
    triples = list(itertools.product(WIDTHS, repeat=3))
    assert set(answers["fin"]) <= {0, 1}
    assert sorted(t for t, a in zip(triples, answers["fin"]) if a == 1) == sorted(FINS)


def test_depthwise_inside(answers):
    for (c, ci), got in zip(itertools.product(WIDTHS, repeat=2), answers["dw"]):
        assert tuple(got) == DW.get((c, ci), (0,) * len(DW_PIXELS)), (c, ci)


def test_adaptor_pairs(answers):
    assert {(c, ci) for _, c, ci in ADAPTORS} <= set(SHAPES)
    triples = list(itertools.product(WIDTHS, repeat=3))
    assert set(answers["pair"]) <= {0, 1}
    assert sorted(t for t, a in zip(triples, answers["pair"]) if a == 1) == sorted(ADAPTORS)


def test_the_two_rules_differ():
    """the numpy restatement of tests/test_block_pack_gpu.py: a closing conv of width 256 (by wave) and dc.0 of an inner width 256
    (by pair) order their tiles differently"""
    assert P.by_wave(256) == [[0], [1], [2], [3], [4], [5], [6], [7]]
    assert P.by_pair(256) == [[0], [2], [4], [6], [1], [3], [5], [7]]
    assert P.by_wave(192) == [[0], [1], [2], [3], [4], [5], [None], [None]]
    assert P.by_pair(384) == [[0, 1], [3, 4], [6, 7], [9, 10], [2], [5], [8], [11]]
    assert P.by_pair(128) == [[0], [1], [2], [3], [], [], [], []] and P.by_wave(128) == [[0], [1], [2], [3], [], [], [], []]
