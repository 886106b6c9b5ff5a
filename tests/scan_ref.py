"""The SCAN rule of DESIGN.md 3.13 in plain numpy int64, vectorised over frames: the reference of
tests/test_scan_gpu.py."""
import numpy as np

INF = 32767


def f(x, y):
    return np.sign(x) * np.sign(y) * np.minimum(np.abs(x), np.abs(y))


def box(x, y):
    return np.where((x == INF) | (y == INF), INF, np.clip(x + y, -32766, 32766))


def scan(mask, llr, iterations):
    """mask [N] (1 = information), llr [B, N] int8 -> (ext [B, N] int64, hard codeword bits [B, N] uint8)"""
    mask, llr, kept = np.asarray(mask).astype(bool), np.asarray(llr).astype(np.int64), {}

    def node(alpha, pos):
        m, h = alpha.shape[1], alpha.shape[1] // 2
        if m == 1:
            return np.full_like(alpha, 0 if mask[pos] else INF)
        a, b = alpha[:, :h], alpha[:, h:]
        left = node(f(a, box(b, kept.get((pos, m), np.zeros_like(b)))), pos)
        right = kept[(pos, m)] = node(box(b, f(a, left)), pos + h)
        beta = np.concatenate([f(left, box(right, b)), box(right, f(left, a))], axis=1)
        for v in (alpha, beta):
            assert v.min() >= -32766 and v.max() <= INF
        return beta

    for _ in range(iterations):
        ext = node(llr, 0)
    return ext, (box(llr, ext) < 0).astype(np.uint8)
