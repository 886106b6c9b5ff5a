"""The list decoder's rule for convolutionally precoded codes ("Precoded codes") in
plain Python, after tests/list_ref.py: recursive over the tree, every path a record holding its own
list of data bits v (list_ref.Path, in its field u), a stable sort on the key tuple."""
import numpy as np

import list_ref
from list_ref import Path, f, g


def precode_np(v, poly, length):
    """u_i = XOR_j c_j v_{i-j} over the rows of v [B, N] (the transmit side, before util.encode_np)"""
    u = np.zeros_like(v)
    for j in (j for j in range(length) if (poly >> j) & 1):
        u[:, j:] ^= v[:, :v.shape[1] - j]
    return u


def walk(paths, alphas, mask, pos, L, poly, length):
    """list_ref.walk with the precoder: the bit sent at a leaf is u = v ^ feed, the fork and the key
    are on the data bit v (frozen: v = 0); returns (paths, partial sums of u, parents)"""
    n = alphas[0].size
    if n == 1:
        cands = []
        for p, al in zip(paths, alphas):
            lam = int(al[0])
            feed = sum(p.u[-j] for j in range(1, min(len(p.u), length - 1) + 1) if (poly >> j) & 1) & 1
            for b in ((0, 1) if mask[pos] else (0,)):
                cands.append(((p.pm + (abs(lam) if (b ^ feed) != (lam < 0) else 0), p.rank, b), p, b ^ feed))
        if mask[pos]:
            cands = sorted(cands, key=lambda c: c[0])[:L]
        out = [Path(k[0], r if mask[pos] else p.rank, p.u + [k[2]]) for r, (k, p, _) in enumerate(cands)]
        return out, [np.array([c[2]], dtype=np.int64) for c in cands], [c[1] for c in cands]
    h = n // 2
    left, bl, par_l = walk(paths, [f(al[:h], al[h:]) for al in alphas], mask, pos, L, poly, length)
    al_l = [alphas[paths.index(p)] for p in par_l]
    right, br, par_r = walk(left, [g(al[:h], al[h:], b) for al, b in zip(al_l, bl)], mask, pos + h, L, poly, length)
    bl_r = [bl[left.index(p)] for p in par_r]
    return right, [np.concatenate([x ^ y, y]) for x, y in zip(bl_r, br)], [par_l[left.index(p)] for p in par_r]


def paths(mask, llr, L, poly, length):
    """per frame, the surviving paths' information bits [count, K] in rank order (no CRC yet)"""
    mask = np.asarray(mask).astype(bool)
    ends = (walk([Path(0, 0, [])], [row.astype(np.int64)], mask, 0, L, poly, length)[0] for row in np.asarray(llr))
    return [np.array([np.array(p.u, np.uint8)[mask] for p in sorted(ps, key=lambda p: p.rank)]) for ps in ends]


def choose(frames, crc_poly=0, crc_len=0):
    """the rule's result from paths(): (info bits [B, K] uint8, rank [B] uint8)"""
    info, rank = [], []
    for bits in frames:
        c = bits.shape[1] - crc_len
        ok = [r for r, b in enumerate(bits) if crc_len and list_ref.crc(b[:c], crc_poly, crc_len) == list(b[c:])]
        info.append(bits[ok[0] if ok else 0])
        rank.append(ok[0] if ok else (0xFF if crc_len else 0))
    return np.array(info), np.array(rank, dtype=np.uint8)
