"""The list decoder's rule restated in plain Python / numpy integers: recursive
over the tree, every path a record of its own, a stable sort on the key tuple, the CRC bit by
bit. It is the checker of tests/test_list_gpu.py and nothing else."""
import numpy as np

GMAX = 32767


def f(a, b):
    return np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b))


def g(a, b, u):
    return np.clip(b + np.where(u == 1, -a, a), -GMAX, GMAX)


def crc(bits, poly, length):
    """register zero, no reflection, no final XOR; returns the check bits, MSB first"""
    reg = 0
    for b in bits:
        fb = ((reg >> (length - 1)) & 1) ^ int(b)
        reg = (reg << 1) & ((1 << length) - 1)
        if fb:
            reg ^= poly
    return [(reg >> (length - 1 - m)) & 1 for m in range(length)]


class Path:
    def __init__(self, pm, rank, u):
        self.pm, self.rank, self.u = pm, rank, u


def walk(paths, alphas, mask, pos, L):
    """decode the node at `pos` whose LLRs are alphas[path index]; returns (paths, betas) with the
    surviving paths in rank order and their partial sums of the node"""
    n = alphas[0].size
    if n == 1:
        cands = []
        for p, al in zip(paths, alphas):
            lam = int(al[0])
            for b in ((0, 1) if mask[pos] else (0,)):
                pm = p.pm + (abs(lam) if b != (lam < 0) else 0)
                cands.append(((pm, p.rank, b), p, b))
        if mask[pos]:
            cands.sort(key=lambda c: c[0])
            cands = cands[:L]
        out = [Path(k[0], r if mask[pos] else p.rank, p.u + [b]) for r, (k, p, b) in enumerate(cands)]
        return out, [np.array([c[2]], dtype=np.int64) for c in cands], [c[1] for c in cands]
    h = n // 2
    left, bl, par_l = walk(paths, [f(al[:h], al[h:]) for al in alphas], mask, pos, L)
    al_l = [alphas[paths.index(p)] for p in par_l]
    right, br, par_r = walk(left, [g(al[:h], al[h:], b) for al, b in zip(al_l, bl)], mask, pos + h, L)
    bl_r = [bl[left.index(p)] for p in par_r]
    beta = [np.concatenate([x ^ y, y]) for x, y in zip(bl_r, br)]
    return right, beta, [par_l[left.index(p)] for p in par_r]


def decode(mask, llr, L, crc_poly=0, crc_len=0):
    """mask [N] 0/1, llr [B, N] int8 -> (info bits [B, K] uint8, rank [B] uint8)"""
    mask = np.asarray(mask).astype(bool)
    K = int(mask.sum())
    info = np.zeros((llr.shape[0], K), dtype=np.uint8)
    rank = np.zeros(llr.shape[0], dtype=np.uint8)
    for fi, row in enumerate(np.asarray(llr)):
        paths, _, _ = walk([Path(0, 0, [])], [row.astype(np.int64)], mask, 0, L)
        paths.sort(key=lambda p: p.rank)
        bits = [np.array(p.u, dtype=np.uint8)[mask] for p in paths]
        pick = 0
        if crc_len:
            ok = [r for r, b in enumerate(bits) if crc(b[:K - crc_len], crc_poly, crc_len) == list(b[K - crc_len:])]
            pick, rank[fi] = (ok[0], ok[0]) if ok else (0, 0xFF)
        info[fi] = bits[pick]
    return info, rank
