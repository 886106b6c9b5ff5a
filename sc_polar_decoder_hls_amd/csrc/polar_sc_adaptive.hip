// polar_sc_adaptive.hip -- the CRC check of adaptive list decoding (gfx950): which
// rows of a batch of information words pass the CRC of the list decoder's rule, and
// the failing rows' indices compacted into a list for the indexed launch of polar_sc_list.hip.
//
// The CRC is linear and its register starts at zero, so a row passes when the remainder of all its
// K information bits (bit 0 first = the highest power of x) is zero. Syndrome bit j is then the
// parity of `row & H_j`, where bit k of H_j is bit j of x^(K-1-k) mod g: c masks of ceil(K/32)
// dwords, built on the host per (K, poly, c) (crc_table below) and kept with the plan.
//
// A wave takes 64 rows, one per lane; waves never synchronise. The rows come in chunks of CH
// dwords: loaded with consecutive lanes on consecutive dwords of a row and staged through the
// wave's share of LDS at a stride of CH + 1 dwords, so that the read-back, lane l reading row l,
// meets no bank twice. The masks of a dword are the same for every lane (scalar loads, CP of them
// side by side); lane l keeps CP accumulators acc_j ^= dword & H_j[w] and passes when none of them
// has odd parity. CP is c rounded up to 8 (four instantiations instead of 32); the rows past c are
// zero, and so are the table's words past ceil(K/32) and bits past K: a row's bits at and above K
// never matter, and every chunk is CH dwords whatever K is.
//
// Compaction: a ballot of the failing lanes, one atomic add per wave on the count, every failing
// lane stores its row index at the wave's base + its prefix count. The order of the list varies
// from run to run. Rows past the batch neither load nor store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_sc_xf.h"

namespace polar_adaptive {

using polar_xf::u32;
using polar_xf::wave_phase;

constexpr int CH = 8;               // dwords of a row per chunk
constexpr int STRIDE = CH + 1;      // of a staged row in LDS (odd: lane-per-row reads spread over all banks)
constexpr int WPB = 4;              // waves per block
constexpr int WAVE_DW = 64 * STRIDE;

// H: [hw][CP] dwords, hw a multiple of CH. info: [batch][rs] dwords. flag (may be null): per row
// `pass_value` when it passes, 1 - pass_value when it fails. zero (may be null): per row a 0 byte
// (the rank of a frame the list decoder does not touch). idx / count (null together): the list.
template <int CP>
__global__ void __launch_bounds__(64 * WPB) polar_sc_crc_check_kernel(
    const u32 *__restrict__ H, const u32 *__restrict__ info, u32 batch, u32 rs, u32 hw, uint8_t *__restrict__ flag,
    u32 pass_value, uint8_t *__restrict__ zero, u32 *__restrict__ idx, u32 *__restrict__ count)
{
    __shared__ u32 lds[WPB * WAVE_DW];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const u32 f0 = (blockIdx.x * (u32)WPB + wave) * 64u;   // (batch <= 2^31 - 8: no wrap)
    if (f0 >= batch) return;                             // (wave-uniform; no block-wide barrier anywhere)
    u32 *my = lds + wave * WAVE_DW;

    u32 acc[CP];
#pragma unroll
    for (int j = 0; j < CP; j++) acc[j] = 0u;
    for (u32 c0 = 0; c0 < hw; c0 += CH) {
#pragma unroll
        for (int i = 0; i < CH; i++) {                   // 64 rows x CH dwords, CH consecutive lanes per row
            const u32 x = lane + 64u * i, row = x / CH, col = x % CH;
            u32 v = 0u;
            if (f0 + row < batch && c0 + col < rs) v = info[(size_t)(f0 + row) * rs + c0 + col];
            my[row * STRIDE + col] = v;
        }
        wave_phase();
#pragma unroll(32 / CP)                                   // (at most 32 masks in scalar registers at a time)
        for (int w = 0; w < CH; w++) {
            const u32 v = my[lane * STRIDE + w];
            const u32 *h = H + (size_t)(c0 + w) * CP;    // (uniform: scalar loads)
#pragma unroll
            for (int j = 0; j < CP; j++) acc[j] ^= v & h[j];
        }
        wave_phase();
    }
    u32 odd = 0u;
#pragma unroll
    for (int j = 0; j < CP; j++) odd |= (u32)__popc(acc[j]);

    const u32 frame = f0 + lane;
    const bool live = frame < batch, fail = live && (odd & 1u);
    if (live) {
        if (flag) flag[frame] = (uint8_t)(fail ? 1u - pass_value : pass_value);
        if (zero) zero[frame] = 0;
    }
    if (!idx) return;
    const unsigned long long votes = __ballot(fail);
    if (!votes) return;
    u32 base = 0u;
    if (lane == 0u) base = atomicAdd(count, (u32)__popcll(votes));
    base = (u32)__builtin_amdgcn_readfirstlane((int)base);
    const u32 at = base + (u32)__popcll(votes & ((1ull << lane) - 1ull));
    if (fail && at < batch) idx[at] = frame;             // (at < batch whenever the count started at zero)
}

// the count of a list, zeroed on the stream (a kernel, not a memset node: the call may be captured)
__global__ void polar_sc_adaptive_clear_kernel(u32 *__restrict__ count)
{
    if (threadIdx.x == 0u) *count = 0u;
}

}  // namespace polar_adaptive

// rows of the table for a CRC of length c (1 .. 32), and its dwords for K information bits
extern "C" uint32_t polar_sc_crc_table_rows(uint32_t c) { return (c + 7u) & ~7u; }
extern "C" size_t polar_sc_crc_table_dwords(uint32_t K, uint32_t c)
{
    const size_t hw = ((size_t)((K + 31u) / 32u) + polar_adaptive::CH - 1) / polar_adaptive::CH * polar_adaptive::CH;
    return hw * polar_sc_crc_table_rows(c);
}

// tab[w][j] (polar_sc_crc_table_dwords of them): bit b = bit j of x^(K-1-k) mod (x^c + poly), k = 32 w + b < K
extern "C" void polar_sc_crc_table(uint32_t K, uint32_t poly, uint32_t c, uint32_t *tab)
{
    const uint32_t cp = polar_sc_crc_table_rows(c);
    const size_t n = polar_sc_crc_table_dwords(K, c);
    for (size_t i = 0; i < n; i++) tab[i] = 0u;
    const uint32_t top = 1u << (c - 1u);
    uint32_t r = 1u;                                     // x^0
    for (uint32_t k = K; k-- > 0u;) {
        for (uint32_t j = 0; j < c; j++)
            if ((r >> j) & 1u) tab[(size_t)(k >> 5) * cp + j] |= 1u << (k & 31u);
        const bool carry = (r & top) != 0u;              // r <- r x mod g
        r = (c == 32u ? r << 1 : (r << 1) & ((1u << c) - 1u)) ^ (carry ? poly : 0u);
    }
}

// Check `batch` rows of rs dwords against the table tab_dev of a CRC of length c. Returns 0 or a
// hipError_t. idx_dev / count_dev non-null: *count_dev is zeroed first, then receives the number of
// failing rows and idx_dev[0 .. *count_dev) their indices (idx_dev holds `batch` entries).
extern "C" int polar_sc_launch_crc_check(const void *tab_dev, const uint64_t *info_dev, size_t batch, uint32_t K,
                                         uint32_t c, uint8_t *flag_dev, uint32_t pass_value, uint8_t *zero_dev,
                                         uint32_t *idx_dev, uint32_t *count_dev, void *stream)
{
    using namespace polar_adaptive;
    hipStream_t s = (hipStream_t)stream;
    const u32 *H = (const u32 *)tab_dev, *info = (const u32 *)info_dev;
    const u32 b = (u32)batch, rs = 2u * ((K + 63u) / 64u), hw = (u32)(polar_sc_crc_table_dwords(K, c) / polar_sc_crc_table_rows(c));
    if (idx_dev) hipLaunchKernelGGL(polar_sc_adaptive_clear_kernel, dim3(1), dim3(64), 0, s, count_dev);
    const dim3 grid((unsigned)((batch + 64u * WPB - 1u) / (64u * WPB))), block(64 * WPB);
    switch (polar_sc_crc_table_rows(c)) {
    case 8: hipLaunchKernelGGL(polar_sc_crc_check_kernel<8>, grid, block, 0, s, H, info, b, rs, hw, flag_dev, pass_value, zero_dev, idx_dev, count_dev); break;
    case 16: hipLaunchKernelGGL(polar_sc_crc_check_kernel<16>, grid, block, 0, s, H, info, b, rs, hw, flag_dev, pass_value, zero_dev, idx_dev, count_dev); break;
    case 24: hipLaunchKernelGGL(polar_sc_crc_check_kernel<24>, grid, block, 0, s, H, info, b, rs, hw, flag_dev, pass_value, zero_dev, idx_dev, count_dev); break;
    default: hipLaunchKernelGGL(polar_sc_crc_check_kernel<32>, grid, block, 0, s, H, info, b, rs, hw, flag_dev, pass_value, zero_dev, idx_dev, count_dev); break;
    }
    return (int)hipGetLastError();
}
