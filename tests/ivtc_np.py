"""Inverse telecine of DESIGN.md 28 (csrc/kernels/ivtc.hip, dcvc_ivtc_*, dcvc encode --ivtc) restated in numpy, in signed
64-bit integers: the GPU tests hold the kernels and the tool against it with ==.

first = the parity of the rows of the field shown first (0 tff, 1 bff), q = 1 - first, t = cthresh << (bits - 8). For a
candidate S in {cur (c), prev (p)}, over the rows y % 2 == q with 1 <= y <= H - 2 and all x, a = cur[y-1][x], b = cur[y+1][x],
s = S[y][x]:
  match_S = sum |2 s - a - b|; comb_S = the number of samples with (s - a > t and s - b > t) or (s - a < -t and s - b < -t);
  blkmax_S = the largest count of such samples in a block (y // 16, x // 32); dup = sum |cur - prev| over all rows y % 2 == first.
Words: [match_c, match_p, comb_c, comb_p, blkmax_c, blkmax_p, dup, 0]; without prev words 1, 3, 5 and 6 are 0.
"""
import numpy as np

import deinterlace_np as dnp
from dcvc_amd.ivtc import Ivtc

I64 = np.int64
BLOCK_H, BLOCK_W = 16, 32
CYCLE = 5


def _measure(S, c, q, t):
    H, W = c.shape
    ys = np.arange(H)
    ys = ys[(ys % 2 == q) & (ys >= 1) & (ys <= H - 2)]
    if ys.size == 0:
        return 0, 0, 0
    a, b, s = c[ys - 1], c[ys + 1], S[ys]
    match = int(np.abs(2 * s - a - b).sum())
    flag = ((s - a > t) & (s - b > t)) | ((s - a < -t) & (s - b < -t))
    counts = np.zeros(((H + BLOCK_H - 1) // BLOCK_H, (W + BLOCK_W - 1) // BLOCK_W), I64)
    yy, xx = np.nonzero(flag)
    np.add.at(counts, (ys[yy] // BLOCK_H, xx // BLOCK_W), 1)
    return match, int(flag.sum()), int(counts.max())


def field_match(cur, prev, first, cthresh, bits):
    """one luma plane and the previous frame's (or None) -> the eight words, Python integers"""
    if first not in (0, 1) or not 0 <= cthresh <= 255 or not 8 <= bits <= 16:
        raise ValueError("first is 0 or 1, cthresh 0..255, bits 8..16")
    c = np.asarray(cur).astype(I64)
    if c.ndim != 2 or c.shape[0] < 2 or c.shape[1] < 1:
        raise ValueError("H >= 2 and W >= 1")
    t = I64(int(cthresh) << (bits - 8))
    q = 1 - first
    words = [0] * 8
    words[0], words[2], words[4] = _measure(c, c, q, t)
    if prev is not None:
        p = np.asarray(prev).astype(I64)
        words[1], words[3], words[5] = _measure(p, c, q, t)
        words[6] = int(np.abs(c[first::2] - p[first::2]).sum())
    return words


def weave_fields(a, b, first):
    """rows of parity first from a, the others from b"""
    out = np.array(b, copy=True)
    out[first::2] = np.asarray(a)[first::2]
    return out


def telecine(film, order, phase=0, seen=None):
    """film: a list of progressive pictures (each a tuple of planes) -> a list of (woven frame, ka, kb) by 2:3 pulldown, ka and
    kb the film pictures of the frame's first and second field. The fields of film picture k are shown 2, 3, 2, 3, ... times,
    starting with the field of the order's parity; `phase` (0..4) drops that many frames off the front, so that the clip starts
    in mid-cadence. seen(i, k): the planes of film picture k as display field i shows them (noise), film[k] by default."""
    first = 0 if order == "tff" else 1
    fields = []                                       # (film index, parity) in display order
    parity = first
    for k in range(len(film)):
        for _ in range(2 if k % 2 == 0 else 3):
            fields.append((k, parity))
            parity = 1 - parity
    frames = []
    for i in range(0, len(fields) - 1, 2):
        (ka, pa), (kb, pb) = fields[i], fields[i + 1]
        assert pa == first and pb == 1 - first
        src_a = film[ka] if seen is None else seen(i, ka)
        src_b = film[kb] if seen is None else seen(i + 1, kb)
        planes = []
        for pl_a, pl_b in zip(src_a, src_b):
            wv = np.empty_like(pl_a)
            wv[pa::2], wv[pb::2] = pl_a[pa::2], pl_b[pb::2]
            planes.append(wv)
        frames.append((tuple(planes), ka, kb))
    return frames[phase:]


def ivtc_clip(frames, mode, order, bits, cthresh=9, mi=80, threshold=10, n=None):
    """frames: woven source frames, each a tuple of planes (luma first) -> (pictures, log). What dcvc encode --ivtc does: every
    frame is measured against its predecessor and pushed; a frame that is not combed is woven from its own first field and the
    second field of itself (c) or of the previous frame (p), a combed one goes through the deinterlacer as --deinterlace
    frame:threshold does; film mode drops, from every complete cycle of 5, the frame dcvc_ivtc_drop names. n: at most n
    pictures are served (frames of a cycle that was begun are still measured). log: per source frame a dict of words, match,
    combed, dropped."""
    if mode not in ("film", "match") or order not in ("tff", "bff"):
        raise ValueError("mode is film or match, order tff or bff")
    first = 0 if order == "tff" else 1
    cycle = CYCLE if mode == "film" else 0
    t = Ivtc(cycle, mi)
    step = CYCLE if mode == "film" else 1
    pictures, log = [], []
    for c0 in range(0, len(frames), step):
        if n is not None and len(pictures) >= n:
            break
        ids = list(range(c0, min(c0 + step, len(frames))))
        for f in ids:
            prev = frames[f - 1] if f > 0 else None
            words = field_match(frames[f][0], None if prev is None else prev[0], first, cthresh, bits)
            r = t.push(f, prev is not None, words)
            log.append({"words": words, "match": "p" if r & 1 else "c", "combed": bool(r & 2), "dropped": False})
        drop = t.drop() if len(ids) == step else -1
        if drop >= 0:
            log[c0 + drop]["dropped"] = True
        for f in ids:
            if log[f]["dropped"] or (n is not None and len(pictures) >= n):
                continue
            prev = frames[f - 1] if f > 0 else None
            if log[f]["combed"]:
                pic = tuple(dnp.deinterlace_plane(pl, None if prev is None else prev[i], first, 0, threshold, bits) for i, pl in enumerate(frames[f]))
            else:
                second = prev if log[f]["match"] == "p" else frames[f]
                pic = tuple(weave_fields(pl, second[i], first) for i, pl in enumerate(frames[f]))
            pictures.append(pic)
    return pictures, log
