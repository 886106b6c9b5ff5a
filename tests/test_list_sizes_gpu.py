"""List decoding on the GPU at the code lengths the other list tests leave out:
N = 64, 256 and 512, i.e. the log2 N = 6, 8 and 9 instantiations of the kernel, with L = 2 and 8 (the
narrow layout) and 16 and 32 (the wide one). N = 512 at L = 32 is the one shape with two waves per
block; N = 256 and 512 are the first lengths where the partial sums have a level above 5 that is not
the last. decode_list against tests/list_ref.py on every bit of the information words and on the rank.

Six frames per case (a partial block at 4 waves per block, several blocks at 2 and 1): four through
AWGN at 1 dB, an all-zero frame (every metric ties), and a noise-free codeword at +-127 with -128
sprinkled in (G at its clamp)."""
import functools

import numpy as np
import pytest

import list_ref
from sc_polar_decoder_hls_amd import _plansets
from test_list_gpu import noisy

MASKS = ("spc_n64", "FB_N256_K128", "FB_N512_K256")
CRC = (0x07, 8)
GUARD = 0x5A


@functools.lru_cache(maxsize=None)
def frames(pkg, name):
    mask = _plansets.soft_mask(name)
    llr, _, x = noisy(pkg, mask, CRC, 6, seed=mask.size + 7)
    llr[-2] = 0
    sprinkle = np.random.default_rng(3).random(mask.size) < 0.3
    llr[-1] = np.where(x[-1] == 1, np.where(sprinkle, -128, -127), 127)
    llr.setflags(write=False)
    return llr


@pytest.mark.gpu
@pytest.mark.parametrize("L", [2, 8, 16, 32])
@pytest.mark.parametrize("name", MASKS)
def test_list_sizes_parity(pkg, cuda, name, L):
    mask = _plansets.soft_mask(name)
    dec = pkg.Decoder(mask)
    llr = frames(pkg, name)
    ref_info, ref_rank = list_ref.decode(mask, llr, L, *CRC)
    B = llr.shape[0]
    buf = cuda.full((B + 1, dec.info_words), 0x5A5A5A5A5A5A5A5A, dtype=cuda.int64, device="cuda")
    rank = cuda.full((B + 1,), GUARD, dtype=cuda.uint8, device="cuda")
    dec.decode_list(cuda.from_numpy(np.array(llr)).cuda(), L, crc=CRC, out=buf[:B], rank=rank[:B])
    got = buf.cpu().numpy().view(np.uint64)
    np.testing.assert_array_equal(got[:B], pkg.pack_bits(ref_info))
    np.testing.assert_array_equal(rank.cpu().numpy()[:B], ref_rank)
    assert (got[B] == 0x5A5A5A5A5A5A5A5A).all() and int(rank[B]) == GUARD      # nothing past the batch
