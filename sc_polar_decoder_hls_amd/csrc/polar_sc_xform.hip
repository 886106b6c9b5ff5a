// polar_sc_xform.hip -- information bits on the device (gfx950): the GF(2) polar transform
// u = x F^{(x)n} on bit-packed frames, fused with a parallel bit compress by the frozen mask
// (extraction, x^ -> information words) or preceded by the parallel bit expand (encoding,
// information words -> codeword). F^{(x)n} is self-inverse and compress / expand by one mask are
// inverses, so both directions share every stage; DESIGN.md 3.8.
//
// Frames are rows of 32-bit dwords (bit i of dword d = x[32 d + i], the x^ format of
// polar_sc_decode read as dwords), D = N / 32 per frame. The Kronecker factors of F^{(x)n}
// commute, so the n butterfly stages run in whatever order the data sits: the five stages
// inside a dword first, then the stages between lanes, then the stages between a lane's
// registers, and for frames of several waves the stages between waves first of all, on the loads.
// A wave never synchronises with another wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_sc_xf.h"

namespace polar_xf {

constexpr int WAVES = 4;              // waves per block; each works alone
constexpr int CHUNK = 2048;           // dwords one wave holds at most (32 registers x 64 lanes)

// inverse of compress: the low popcount(m) bits of x spread to the positions of e.m
__device__ __forceinline__ u32 expand(u32 x, const Ent &e)
{
#pragma unroll
    for (int i = 4; i >= 0; i--) {
        const u32 t = x << (1 << i);
        x = (x & ~e.mv[i]) | (t & e.mv[i]);
    }
    return x & e.m;
}

// one stage between lanes: the lane with the distance bit clear takes w ^= w of lane + DIST;
// the other lane of the pair keeps its value
template <int DIST>
__device__ __forceinline__ u32 xf_lane_stage(u32 w, u32 lane)
{
    if constexpr (DIST == 1) {
        const u32 p = __builtin_amdgcn_update_dpp(0u, w, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
        return w ^ ((lane & 1u) ? 0u : p);
    } else if constexpr (DIST == 2) {
        const u32 p = __builtin_amdgcn_update_dpp(0u, w, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
        return w ^ ((lane & 2u) ? 0u : p);
    } else if constexpr (DIST == 4) {
        // row_shl:4 into banks 0 and 2 (lanes 0..3, 8..11 of each row); the others read 0
        return w ^ __builtin_amdgcn_update_dpp(0u, w, 0x104, 0xF, 0x5, false);
    } else if constexpr (DIST == 8) {
        // row_shl:8 into banks 0 and 1 (lanes 0..7 of each row)
        return w ^ __builtin_amdgcn_update_dpp(0u, w, 0x108, 0xF, 0x3, false);
    } else if constexpr (DIST == 16) {
        const auto s = __builtin_amdgcn_permlane16_swap(w, w, false, false);   // s[1]: rows (1 1 3 3)
        return w ^ ((lane & 16u) ? 0u : s[1]);
    } else {
        const auto s = __builtin_amdgcn_permlane32_swap(w, w, false, false);   // s[1]: halves (1 1)
        return w ^ ((lane & 32u) ? 0u : s[1]);
    }
}

// the stages of dword distance 1 .. DL / 2 among DL consecutive lanes
template <int DL>
__device__ __forceinline__ u32 xf_lanes(u32 w, u32 lane)
{
    if constexpr (DL > 1) w = xf_lane_stage<1>(w, lane);
    if constexpr (DL > 2) w = xf_lane_stage<2>(w, lane);
    if constexpr (DL > 4) w = xf_lane_stage<4>(w, lane);
    if constexpr (DL > 8) w = xf_lane_stage<8>(w, lane);
    if constexpr (DL > 16) w = xf_lane_stage<16>(w, lane);
    if constexpr (DL > 32) w = xf_lane_stage<32>(w, lane);
    return w;
}

// encode prologue: the popcount(m) information bits of a dword, from bit e.off of the frame's
// information row (at most two dwords; neither is read unless the mask says it holds a bit)
__device__ __forceinline__ u32 gather_info(const u32 *__restrict__ irow, const Ent &e)
{
    const u32 sh = e.off & 31u, q = e.off >> 5;
    const u32 lo = e.pc ? irow[q] : 0u;
    const u32 hi = (sh + e.pc > 32u) ? irow[q + 1] : 0u;
    const u32 v = __builtin_amdgcn_alignbit(hi, lo, sh);     // ({hi, lo} >> sh), sh = 0: lo
    return e.pc ? (v & (0xFFFFFFFFu >> (32u - e.pc))) : 0u;
}

// extract epilogue: OR the compressed piece c of a dword into the LDS image of the wave's
// output range (seg[0] = the dword that holds information bit 32 * q0)
__device__ __forceinline__ void scatter_info(u32 *seg, u32 q0, u32 c, const Ent &e)
{
    const u32 sh = e.off & 31u, q = (e.off >> 5) - q0;
    if (e.pc) atomicOr(&seg[q], c << sh);
    if (sh + e.pc > 32u) atomicOr(&seg[q + 1], c >> (32u - sh));   // (sh > 0 here)
}

// ---------------------------------------------------------------------------------------
// N <= 2048: one dword per lane, 64 / D consecutive frames per wave
//   x rows: max(D, 2) dwords (N = 32: a half-used u64), information rows: irow dwords
// ---------------------------------------------------------------------------------------
template <int LOGD, bool ENC>
__global__ void __launch_bounds__(64 * WAVES) polar_sc_xform_small_kernel(
    const Ent *__restrict__ tab, const u32 *__restrict__ in, u32 *__restrict__ out, u32 batch, u32 irow)
{
    constexpr int D = 1 << LOGD, FPW = 64 >> LOGD, XROW = D < 2 ? 2 : D;
    __shared__ u32 img_all[ENC ? 1 : WAVES * 128];   // per wave: FPW rows of irow <= XROW dwords
    const size_t gl = (size_t)blockIdx.x * (64u * WAVES) + threadIdx.x;
    const size_t frame = gl >> LOGD;
    const u32 d = (u32)gl & (u32)(D - 1), lane = threadIdx.x & 63u;
    const bool valid = frame < batch;
    const Ent e = load_ent(tab, d);
    if constexpr (ENC) {
        u32 w = valid ? gather_info(in + frame * irow, e) : 0u;
        w = xf_lanes<D>(xf_dword(expand(w, e)), lane);
        if (valid) {
            if constexpr (D == 1) *(uint2 *)(out + frame * 2u) = make_uint2(w, 0u);
            else out[frame * XROW + d] = w;
        }
    } else {
        u32 *img = img_all + (threadIdx.x >> 6) * 128u;
        img[lane] = 0u;
        img[lane + 64u] = 0u;
        u32 w = valid ? in[frame * XROW + d] : 0u;
        w = xf_lanes<D>(xf_dword(w), lane);
        const u32 c = compress(w, e);
        wave_phase();
        scatter_info(img + (lane >> LOGD) * irow, 0u, c, e);
        wave_phase();
        const size_t f0 = (gl - lane) >> LOGD;       // the wave's first frame
        const u32 total = FPW * irow;                // <= 128
        for (u32 i = lane; i < total; i += 64u)
            if (f0 + i / irow < batch) out[f0 * irow + i] = img[i];
    }
}

// ---------------------------------------------------------------------------------------
// Precoded encoding, N <= 1024 (the list decoder's range; DESIGN.md 3.11 "Precoded codes"): the
// encode path above with the convolutional precoder between the expand and the transform. v = the
// expanded information bits, u_i = XOR over the taps c_j of v_{i-j}: on packed bits, dword d of u is
// the XOR over the taps of {v[d], v[d-1]} shifted by j, and v[d-1] is the lane below (conv_len <= 32,
// so no tap reaches further). cpoly: bit j = c_j, c_0 = 1.
// ---------------------------------------------------------------------------------------
template <int LOGD>
__global__ void __launch_bounds__(64 * WAVES) polar_sc_encode_precoded_kernel(
    const Ent *__restrict__ tab, const u32 *__restrict__ in, u32 *__restrict__ out, u32 batch, u32 irow, u32 cpoly)
{
    constexpr int D = 1 << LOGD, XROW = D < 2 ? 2 : D;
    const size_t gl = (size_t)blockIdx.x * (64u * WAVES) + threadIdx.x;
    const size_t frame = gl >> LOGD;
    const u32 d = (u32)gl & (u32)(D - 1), lane = threadIdx.x & 63u;
    const bool valid = frame < batch;
    const Ent e = load_ent(tab, d);
    const u32 v = expand(valid ? gather_info(in + frame * irow, e) : 0u, e);
    // wave_shr:1, lane l takes lane l - 1 (lane 0: 0); dword 0 of a frame has nothing before it
    const u32 below = __builtin_amdgcn_update_dpp(0u, v, 0x138, 0xF, 0xF, true);
    const u32 prev = d ? below : 0u;
    u32 u = v;                                                   // tap 0
    for (u32 c = cpoly & ~1u; c; c &= c - 1u)                    // (uniform: the set taps 1 .. 31)
        u ^= __builtin_amdgcn_alignbit(v, prev, 32u - (u32)__builtin_ctz(c));   // ({v, prev} >> (32 - j))
    const u32 w = xf_lanes<D>(xf_dword(u), lane);
    if (valid) {
        if constexpr (D == 1) *(uint2 *)(out + frame * 2u) = make_uint2(w, 0u);
        else out[frame * XROW + d] = w;
    }
}

// ---------------------------------------------------------------------------------------
// 2048 < N <= 65536: one wave per frame, dword d = 64 r + lane in register r (R = D / 64).
// N >= 131072 (MULTI): wave c of a frame's W = N / 65536 owns the 65536-bit chunk c; the
// stages between chunks run on the loads (chunk c of the result is the XOR of every chunk c'
// whose index is a bit-superset of c), then the single-wave code runs on the chunk.
// ---------------------------------------------------------------------------------------
template <int R>
__device__ __forceinline__ void xf_chunk(u32 (&reg)[R], u32 lane)
{
#pragma unroll
    for (int r = 0; r < R; r++) reg[r] = xf_lanes<64>(xf_dword(reg[r]), lane);
#pragma unroll
    for (int h = 1; h < R; h <<= 1)
#pragma unroll
        for (int r = 0; r < R; r++)
            if (!(r & h)) reg[r] ^= reg[r + h];
}

template <int R, bool ENC, bool MULTI>
__global__ void __launch_bounds__(64 * WAVES) polar_sc_xform_wave_kernel(
    const Ent *__restrict__ tab, const u32 *__restrict__ in, u32 *__restrict__ out, u32 batch, u32 irow,
    u32 K, u32 logW)
{
    static_assert(!MULTI || R * 64 == CHUNK, "multi-wave frames: full chunks");
    constexpr int IMG = ENC ? 1 : R * 64 + 2;    // a chunk's range of <= 64 R bits at any bit offset
    __shared__ u32 img_all[ENC ? 1 : WAVES * IMG];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t gw = (size_t)blockIdx.x * WAVES + wave;
    const u32 W = 1u << logW;
    const size_t frame = MULTI ? gw >> logW : gw;
    const u32 c = MULTI ? (u32)gw & (W - 1u) : 0u;
    if (frame >= batch) return;                  // (wave-uniform; no block-wide barrier anywhere)
    const size_t xdw = (size_t)(R * 64) << (MULTI ? logW : 0u);   // dwords of an x row
    const u32 d0 = c * (u32)(R * 64);            // the wave's first dword
    const u32 free_bits = MULTI ? ~c & (W - 1u) : 0u;
    u32 reg[R];
#pragma unroll
    for (int r = 0; r < R; r++) reg[r] = 0u;
    if constexpr (ENC) {
        const u32 *irp = in + frame * irow;
        for (u32 s = free_bits;; s = (s - 1u) & free_bits) {     // c' = c | s over the supersets of c
            const u32 dd = (c | s) * (u32)(R * 64);
#pragma unroll
            for (int r = 0; r < R; r++) {
                const Ent e = load_ent(tab, dd + 64u * r + lane);
                reg[r] ^= expand(gather_info(irp, e), e);
            }
            if (s == 0u) break;
        }
        xf_chunk<R>(reg, lane);
        u32 *xo = out + frame * xdw + d0;
#pragma unroll
        for (int r = 0; r < R; r++) xo[64u * r + lane] = reg[r];
    } else {
        const u32 *xi = in + frame * xdw;
        for (u32 s = free_bits;; s = (s - 1u) & free_bits) {
            const u32 dd = (c | s) * (u32)(R * 64);
#pragma unroll
            for (int r = 0; r < R; r++) reg[r] ^= xi[dd + 64u * r + lane];
            if (s == 0u) break;
        }
        xf_chunk<R>(reg, lane);
        u32 *img = img_all + wave * IMG;
        for (u32 i = lane; i < (u32)IMG; i += 64u) img[i] = 0u;
        // the chunk's information bits are [beg, end) of the frame's
        const u32 beg = MULTI ? tab[d0].off : 0u;
        const u32 end = (MULTI && c + 1u < W) ? tab[d0 + R * 64].off : K;
        const u32 q0 = beg >> 5;
        wave_phase();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const Ent e = load_ent(tab, d0 + 64u * r + lane);
            scatter_info(img, q0, compress(reg[r], e), e);
        }
        wave_phase();
        u32 *orow = out + frame * irow;
        if constexpr (!MULTI) {
            // the whole row, zero padding of the last u64 included (irow <= 64 R)
            for (u32 i = lane; i < irow; i += 64u) orow[i] = img[i];
        } else if (end > beg) {
            // the first and the last dword of the range may hold a neighbour chunk's bits too: those
            // two go out with a vector atomic OR into the row the launcher cleared
            const u32 n = ((end - 1u) >> 5) - q0 + 1u;   // <= 64 R + 1
            for (u32 i = lane; i < n; i += 64u) {
                if (i == 0u || i == n - 1u) atomicOr(&orow[q0 + i], img[i]);
                else orow[q0 + i] = img[i];
            }
        }
    }
}

// clears n u64 words (the rows that chunks of one frame then OR into; not a memset node, so
// that the call can be captured into a graph)
__global__ void __launch_bounds__(256) polar_sc_xform_clear_kernel(uint2 *__restrict__ p, size_t n)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i < n) p[i] = make_uint2(0u, 0u);
}

}  // namespace polar_xf

// ---------------------------------------------------------------------------------------
// host: the plan's table, and launch glue (called from polar_sc_host.cpp)
// ---------------------------------------------------------------------------------------
// tab: max(1, N / 32) records of 8 dwords (polar_xf::Ent) from the information mask (N bytes)
extern "C" void polar_sc_xform_table(const uint8_t *mask, uint32_t N, uint32_t *tab)
{
    uint32_t off = 0;
    for (uint32_t d = 0; d < N / 32u; d++) {
        uint32_t m = 0;
        for (uint32_t i = 0; i < 32u; i++) m |= (uint32_t)(mask[32u * d + i] != 0) << i;
        uint32_t *e = tab + 8u * d;
        const uint32_t pc = (uint32_t)__builtin_popcount(m);
        e[0] = m;
        e[1] = off;
        e[7] = pc;
        off += pc;
        uint32_t mk = ~m << 1;
        for (int i = 0; i < 5; i++) {
            uint32_t mp = mk ^ (mk << 1);                  // parallel suffix
            mp ^= mp << 2;
            mp ^= mp << 4;
            mp ^= mp << 8;
            mp ^= mp << 16;
            const uint32_t mv = mp & m;                    // bits to move by 2^i
            m = (m ^ mv) | (mv >> (1 << i));
            mk &= ~mp;
            e[2 + i] = mv;
        }
    }
}

namespace {

template <bool ENC>
void launch_small(int logD, unsigned blocks, hipStream_t s, const polar_xf::Ent *tab, const uint32_t *in, uint32_t *out,
                  uint32_t batch, uint32_t irow)
{
    const dim3 g(blocks), b(64 * polar_xf::WAVES);
    switch (logD) {
#define POLAR_XF_CASE(L)                                                                                        \
    case L:                                                                                                     \
        hipLaunchKernelGGL((polar_xf::polar_sc_xform_small_kernel<L, ENC>), g, b, 0, s, tab, in, out, batch, irow); \
        break;
        POLAR_XF_CASE(0) POLAR_XF_CASE(1) POLAR_XF_CASE(2) POLAR_XF_CASE(3) POLAR_XF_CASE(4) POLAR_XF_CASE(5)
        POLAR_XF_CASE(6)
#undef POLAR_XF_CASE
    }
}

template <bool ENC>
void launch_wave(int R, unsigned blocks, hipStream_t s, const polar_xf::Ent *tab, const uint32_t *in, uint32_t *out,
                 uint32_t batch, uint32_t irow, uint32_t K, uint32_t logW)
{
    const dim3 g(blocks), b(64 * polar_xf::WAVES);
    if (logW) {
        hipLaunchKernelGGL((polar_xf::polar_sc_xform_wave_kernel<32, ENC, true>), g, b, 0, s, tab, in, out, batch, irow,
                           K, logW);
        return;
    }
    switch (R) {
#define POLAR_XF_CASE(RR)                                                                                    \
    case RR:                                                                                                 \
        hipLaunchKernelGGL((polar_xf::polar_sc_xform_wave_kernel<RR, ENC, false>), g, b, 0, s, tab, in, out, batch, \
                           irow, K, 0u);                                                                     \
        break;
        POLAR_XF_CASE(2) POLAR_XF_CASE(4) POLAR_XF_CASE(8) POLAR_XF_CASE(16) POLAR_XF_CASE(32)
#undef POLAR_XF_CASE
    }
}

}  // namespace

// clear n u64 words on the stream; returns 0, a hipError_t, or -1 (too large for one grid)
extern "C" int polar_sc_launch_xform_clear(uint64_t *p_dev, size_t n, void *stream)
{
    if (n == 0) return 0;
    const size_t blocks = (n + 255u) / 256u;
    if (blocks > 0x7FFFFFFFu) return -1;
    hipLaunchKernelGGL(polar_xf::polar_sc_xform_clear_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (uint2 *)p_dev, n);
    return (int)hipGetLastError();
}

// information rows -> codeword rows of the code precoded with conv_poly (bit j = c_j, c_0 = 1, judged
// by the caller). 32 <= N <= 1024 a power of two, 1 <= K <= N, 1 <= batch <= 2^31 - 8. Returns as
// polar_sc_launch_xform_clear.
extern "C" int polar_sc_launch_encode_precoded(const void *tab_dev, const uint64_t *in_dev, uint64_t *out_dev, uint32_t N,
                                               uint32_t K, size_t batch, uint32_t conv_poly, void *stream)
{
    int logD = 0;
    while ((32u << logD) < N) logD++;
    if (logD > 5) return (int)hipErrorInvalidValue;
    const size_t blocks = ((batch << logD) + 64u * polar_xf::WAVES - 1u) / (64u * polar_xf::WAVES);
    if (blocks > 0x7FFFFFFFu) return -1;
    const dim3 g((unsigned)blocks), b(64 * polar_xf::WAVES);
    switch (logD) {
#define POLAR_XF_CASE(L)                                                                                       \
    case L:                                                                                                    \
        hipLaunchKernelGGL((polar_xf::polar_sc_encode_precoded_kernel<L>), g, b, 0, (hipStream_t)stream,       \
                           (const polar_xf::Ent *)tab_dev, (const uint32_t *)in_dev, (uint32_t *)out_dev,      \
                           (uint32_t)batch, 2u * ((K + 63u) / 64u), conv_poly);                                \
        break;
        POLAR_XF_CASE(0) POLAR_XF_CASE(1) POLAR_XF_CASE(2) POLAR_XF_CASE(3) POLAR_XF_CASE(4) POLAR_XF_CASE(5)
#undef POLAR_XF_CASE
    }
    return (int)hipGetLastError();
}

// encode = 0: in = x^ rows, out = information rows; encode = 1: the reverse. 32 <= N <= 2^20 a
// power of two, 1 <= K <= N, 1 <= batch <= 2^31 - 8. Returns as polar_sc_launch_xform_clear.
extern "C" int polar_sc_launch_xform(int encode, const void *tab_dev, const uint64_t *in_dev, uint64_t *out_dev,
                                     uint32_t N, uint32_t K, size_t batch, void *stream)
{
    const polar_xf::Ent *tab = (const polar_xf::Ent *)tab_dev;
    const uint32_t *in = (const uint32_t *)in_dev;
    uint32_t *out = (uint32_t *)out_dev;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t irow = 2u * ((K + 63u) / 64u);
    int logD = 0;
    while ((32u << logD) < N) logD++;
    if (logD <= 6) {
        const size_t blocks = ((batch << logD) + 64u * polar_xf::WAVES - 1u) / (64u * polar_xf::WAVES);
        if (blocks > 0x7FFFFFFFu) return -1;
        if (encode) launch_small<true>(logD, (unsigned)blocks, s, tab, in, out, (uint32_t)batch, irow);
        else launch_small<false>(logD, (unsigned)blocks, s, tab, in, out, (uint32_t)batch, irow);
        return (int)hipGetLastError();
    }
    const uint32_t logW = logD > 11 ? (uint32_t)(logD - 11) : 0u;
    const size_t blocks = ((batch << logW) + polar_xf::WAVES - 1u) / polar_xf::WAVES;
    if (blocks > 0x7FFFFFFFu) return -1;
    if (logW && !encode) {   // chunks of one frame OR their boundary dwords into the row
        const int rc = polar_sc_launch_xform_clear(out_dev, batch * (size_t)(irow / 2u), stream);
        if (rc) return rc;
    }
    const int R = 1 << (logD - 6 - (int)logW);
    if (encode) launch_wave<true>(R, (unsigned)blocks, s, tab, in, out, (uint32_t)batch, irow, K, logW);
    else launch_wave<false>(R, (unsigned)blocks, s, tab, in, out, (uint32_t)batch, irow, K, logW);
    return (int)hipGetLastError();
}
