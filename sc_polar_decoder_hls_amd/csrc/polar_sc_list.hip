// polar_sc_list.hip -- successive-cancellation list decoding (gfx950): the L best paths of the SC
// tree, ranked by an integer path metric, with an optional CRC inside the payload choosing the
// survivor; int8 LLRs in, information words out, one launch. DESIGN.md 3.11 defines the decoding
// rule; this file follows it bit for bit.
//
// One wave decodes one frame; waves never synchronise with each other. All state of a frame lives
// in the wave's share of LDS:
//   R        the channel LLRs as int16 (level LOGN of the tree, shared by every path)
//   A[p][s]  LLR arrays: level s (a node of 2^s LLRs) of physical array p, int16, at element 2^s
//   B[p][s]  partial sums of the completed left child at level s of physical array p, bit-packed
//   T        per rank: path metric, the two index words below, the bit decided last
// Paths share arrays through two index words per rank (3 bits per level): word `a` names the
// physical array that holds the path's LLRs of each level, word `b` the same for the partial sums.
// Every live path walks the tree in lockstep, so a level is rewritten by all paths at once: what
// the level held before is dead for every path, and rank j simply takes physical array j for it.
// A fork therefore copies two index words and nothing else; no level is ever copied, no
// reference is counted, no array is allocated.
//
// The walk is bit by bit (no node shortcuts). Leaf i first recomputes the levels below the lowest
// set bit t of i: G of level t from the parent's arrays (wherever the index word says they are),
// then F down to level 1, packed two int16 per lane; the leaf LLR itself is F or G of the level-1
// pair, taken in a register. An information leaf ranks its 2 * paths candidates by the key
// PM' << 4 | rank << 1 | bit (unique, so counting the smaller keys is the destination rank) and
// scatters the survivors' state to their new ranks. Then the decided bits are folded into the
// partial sums: beta = (left ^ right, right) level by level up to the first level that is a left
// child, where it is stored. After the last leaf that is the level-LOGN array: the codeword
// estimate of every path, from which the information words come as in polar_sc_xform.hip
// (transform, compress by the mask with the plan's per-dword table, OR into an LDS image).
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace polar_list {

typedef uint32_t u32;
typedef short s16x2 __attribute__((ext_vector_type(2)));

// the per-dword record of the plan's transform table (polar_sc_xform.hip polar_xf::Ent)
struct __attribute__((aligned(32))) Ent {
    u32 m, off, mv[5], pc;
};

constexpr int GMAX = 32767;     // |G| bound of the rule

// dword of level s inside a path's partial-sum array: levels 0..4 take a dword each, level
// s >= 5 takes 2^(s-5)
__host__ __device__ constexpr int boff(int s) { return s < 5 ? s : 4 + (1 << (s - 5)); }

template <int LOGN, int L>
struct Shape {
    static constexpr int N = 1 << LOGN;
    static constexpr int D = N / 32;                  // dwords of a codeword
    static constexpr int R_DW = N / 2;                // channel LLRs, int16
    static constexpr int A_DW = N / 2;                // per physical array: levels 1 .. LOGN-1 (+ pad)
    static constexpr int B_DW = boff(LOGN) + D;       // levels 0 .. LOGN
    static constexpr int T_DW = 2 * 4 * L;            // two copies of {pm, a, b, bit}[L]
    static constexpr int WAVE_DW = R_DW + L * A_DW + L * B_DW + T_DW;
    // waves per block: 4 where they fit the 64 KB of a block's static LDS, else 1 (a CU holds
    // 160 KB: single-wave blocks leave the least of it unused)
    static constexpr int WPB = WAVE_DW * 4 * 4 <= 65536 ? 4 : 1;
    static constexpr int IROW = D < 2 ? 2 : D;        // information-row image per path (dwords), inside A
    static_assert(IROW <= A_DW, "the information image reuses the LLR arrays");
};

// orders the phases of the wave's LDS state: LDS executes one wave's instructions in order, so only
// the compiler has to be held
__device__ __forceinline__ void wave_phase()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ s16x2 as_pk(u32 x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u32 as_u(s16x2 x) { return __builtin_bit_cast(u32, x); }
// (no operand is ever -32768: the channel is int8 and G clamps at +-32767)
__device__ __forceinline__ s16x2 pk_abs(s16x2 v) { return __builtin_elementwise_max(v, -v); }

// F of two LLR pairs: sign(a) sign(b) min(|a|, |b|); min gives the 0 of a zero operand
__device__ __forceinline__ u32 f_pk(u32 a, u32 b)
{
    const s16x2 va = as_pk(a), vb = as_pk(b);
    const s16x2 m = __builtin_elementwise_min(pk_abs(va), pk_abs(vb));
    const s16x2 sg = (va ^ vb) >> 15;
    return as_u((m ^ sg) - sg);
}

// G of two LLR pairs, u = bits 0 and 1: clamp(b + (u ? -a : a)); the saturating packed add stops at
// -32768, the max brings that to -32767
__device__ __forceinline__ u32 g_pk(u32 a, u32 b, u32 u)
{
    const s16x2 um = as_pk(((0u - (u & 1u)) & 0xFFFFu) | ((0u - ((u >> 1) & 1u)) << 16));
    const s16x2 sa = (as_pk(a) ^ um) - um;
    const s16x2 lo = {-GMAX, -GMAX};
    return as_u(__builtin_elementwise_max(__builtin_elementwise_add_sat(as_pk(b), sa), lo));
}

__device__ __forceinline__ int f_one(int a, int b)
{
    const int m = min(abs(a), abs(b));
    return ((a ^ b) < 0) ? -m : m;
}

__device__ __forceinline__ int g_one(int a, int b, u32 u)
{
    return min(max(b + (u ? -a : a), -GMAX), GMAX);   // (one v_med3_i32)
}

__device__ __forceinline__ u32 field(u32 w, int s) { return (w >> (3 * s)) & 7u; }

// bits under e.m packed at the low end (polar_sc_xform.hip compress)
__device__ __forceinline__ u32 compress(u32 x, const Ent &e)
{
    x &= e.m;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        const u32 t = x & e.mv[i];
        x = (x ^ t) | (t >> (1 << i));
    }
    return x;
}

__device__ __forceinline__ Ent load_ent(const Ent *__restrict__ tab, u32 d)
{
    const uint4 *q = (const uint4 *)(tab + d);
    const uint4 a = q[0], b = q[1];
    Ent e;
    e.m = a.x; e.off = a.y; e.mv[0] = a.z; e.mv[1] = a.w;
    e.mv[2] = b.x; e.mv[3] = b.y; e.mv[4] = b.z; e.pc = b.w;
    return e;
}

// The state of one frame; every member function is called by the whole wave.
template <int LOGN, int L>
struct Wave {
    typedef Shape<LOGN, L> S;
    u32 *R, *A, *B, *T;
    u32 lane;
    int count;      // live paths (wave-uniform)
    int cur;        // which copy of T is current

    __device__ __forceinline__ u32 *tab_pm(int c) { return T + c * 4 * L; }
    __device__ __forceinline__ u32 *tab_a(int c) { return T + c * 4 * L + L; }
    __device__ __forceinline__ u32 *tab_b(int c) { return T + c * 4 * L + 2 * L; }
    __device__ __forceinline__ u32 *tab_bit(int c) { return T + c * 4 * L + 3 * L; }

    // level s (1 <= s < LOGN) of every live path from level s + 1: count * 2^(s-1) LLR pairs over
    // the 64 lanes. F reads the path's own array (written by the step before) or, at the top, the
    // channel; G reads the array the index word names and the partial sums of its left child.
    template <bool IS_G>
    __device__ __forceinline__ void node(int s)
    {
        const int sh = s - 1, half = 1 << sh, total = count << sh;
        for (int w = (int)lane; w < total; w += 64) {
            const int j = w >> sh, e = w & (half - 1);
            const u32 *in;
            u32 u = 0;
            if (s + 1 == LOGN) {
                in = R;
            } else {
                const u32 p = IS_G ? field(tab_a(cur)[j], s + 1) : (u32)j;
                in = A + p * S::A_DW + (1 << s);
            }
            if (IS_G) {
                const u32 q = field(tab_b(cur)[j], s);
                u = B[q * S::B_DW + boff(s) + (e >> 4)] >> ((2 * e) & 31);
            }
            const u32 a = in[e], b = in[e + half];
            A[j * S::A_DW + half + e] = IS_G ? g_pk(a, b, u) : f_pk(a, b);
        }
        wave_phase();
    }

    // the LLR of leaf i for path r (r < count): F or G of the level-1 pair
    __device__ __forceinline__ int leaf_llr(u32 i, u32 r)
    {
        if (!(i & 1u)) {
            const u32 v = A[r * S::A_DW + 1];
            return f_one((short)(v & 0xFFFFu), (short)(v >> 16));
        }
        const u32 v = A[field(tab_a(cur)[r], 1) * S::A_DW + 1];
        const u32 u = B[field(tab_b(cur)[r], 0) * S::B_DW] & 1u;
        return g_one((short)(v & 0xFFFFu), (short)(v >> 16), u);
    }

    __device__ __forceinline__ void frozen_leaf(u32 i)
    {
        if ((int)lane < count) {
            const int lam = leaf_llr(i, lane);
            tab_pm(cur)[lane] += lam < 0 ? (u32)(-lam) : 0u;
            tab_bit(cur)[lane] = 0u;
        }
        wave_phase();
    }

    // candidates 2 r + bit in lanes 0 .. 2 count - 1; the survivors go to the other copy of T
    __device__ __forceinline__ void info_leaf(u32 i)
    {
        const u32 r = lane >> 1, bit = lane & 1u;
        const bool valid = (int)r < count;
        u32 key = 0xFFFFFFFFu, pm = 0, ia = 0, ib = 0;
        if (valid) {
            const int lam = leaf_llr(i, r);
            ia = tab_a(cur)[r];
            ib = tab_b(cur)[r];
            pm = tab_pm(cur)[r] + (bit != (u32)(lam < 0) ? (u32)abs(lam) : 0u);
            key = (pm << 4) | (r << 1) | bit;
        }
        u32 dest = 0;
#pragma unroll
        for (int k = 0; k < 2 * L; k++) dest += (u32)__builtin_amdgcn_readlane((int)key, k) < key ? 1u : 0u;
        const int nxt = cur ^ 1;
        if (valid && dest < (u32)L) {
            tab_pm(nxt)[dest] = pm;
            tab_a(nxt)[dest] = ia;
            tab_b(nxt)[dest] = ib;
            tab_bit(nxt)[dest] = bit;
        }
        cur = nxt;
        count = min(L, 2 * count);
        wave_phase();
    }

    // fold the bit decided at leaf i into the partial sums: t = the level of the first ancestor that
    // is a left child (LOGN after the last leaf). Levels below 5 fold in a register of lane j =
    // rank j; higher ones in place in the destination, one dword per lane. Then rank j owns array j
    // for that level of the partial sums and for the LLR levels 1 .. t the next leaf rewrites.
    __device__ __forceinline__ void fold_bits(u32 i)
    {
        const int t = (i + 1u == (u32)S::N) ? LOGN : __builtin_ctz(i + 1u);
        const bool live = (int)lane < count;
        u32 ib = 0;
        if (live) {
            ib = tab_b(cur)[lane];
            u32 beta = tab_bit(cur)[lane];
            const int ts = t < 5 ? t : 5;
            for (int s = 0; s < ts; s++) {
                const u32 bl = B[field(ib, s) * S::B_DW + s];
                beta = (bl ^ beta) | (beta << (1 << s));
            }
            B[lane * S::B_DW + boff(t)] = beta;
        }
        wave_phase();
        for (int s = 5; s < t; s++) {
            const int sh = s - 5, w = 1 << sh, total = count << sh;
            for (int x = (int)lane; x < total; x += 64) {
                const int j = x >> sh, d = x & (w - 1);
                u32 *dst = B + j * S::B_DW + boff(t);
                const u32 c = dst[d];
                dst[d] = c ^ B[field(tab_b(cur)[j], s) * S::B_DW + boff(s) + d];
                dst[w + d] = c;
            }
            wave_phase();
        }
        if (live && t < LOGN) {
            constexpr u32 ONES = 01111111111u;                  // a 1 in every 3-bit field
            const u32 am = ((1u << (3 * t + 3)) - 1u) & ~7u;    // fields 1 .. t
            tab_a(cur)[lane] = (tab_a(cur)[lane] & ~am) | ((lane * ONES) & am);
            tab_b(cur)[lane] = (ib & ~(7u << (3 * t))) | (lane << (3 * t));
        }
        wave_phase();
    }
};

// dwords of a codeword through u = x F^{(x)n}: the five stages inside a dword
__device__ __forceinline__ u32 xf_dword(u32 w)
{
    w ^= (w >> 1) & 0x55555555u;
    w ^= (w >> 2) & 0x33333333u;
    w ^= (w >> 4) & 0x0F0F0F0Fu;
    w ^= (w >> 8) & 0x00FF00FFu;
    w ^= (w >> 16) & 0x0000FFFFu;
    return w;
}

// CRC of the rule over an information row in LDS: register zero, no reflection, no final XOR;
// message = bits 0 .. K-c-1 MSB first, check = bits K-c .. K-1 MSB first. One lane per path.
__device__ __forceinline__ bool crc_passes(const u32 *row, u32 K, u32 poly, u32 c)
{
    const u32 top = 1u << (c - 1u), keep = c == 32u ? 0xFFFFFFFFu : (1u << c) - 1u;
    const u32 msg = K - c;
    u32 reg = 0, w = 0;
    for (u32 k = 0; k < msg; k++) {
        if (!(k & 31u)) w = row[k >> 5];
        const u32 fb = ((reg & top) ? 1u : 0u) ^ (w & 1u);
        w >>= 1;
        reg = ((reg << 1) & keep) ^ (fb ? poly : 0u);
    }
    u32 bad = 0;
    for (u32 m = 0; m < c; m++) {
        const u32 k = msg + m;
        bad |= ((row[k >> 5] >> (k & 31u)) ^ (reg >> (c - 1u - m))) & 1u;
    }
    return bad == 0u;
}

// INDEXED = false: the direct launch, wave slot f decodes frame f of the batch (idx and count unused).
// INDEXED = true: the indexed launch of adaptive decoding: the frames to decode are
// idx[0 .. *idx_count), a list only the device knows (polar_sc_adaptive.hip wrote it earlier on the
// stream). The grid still has a wave slot per frame of the batch; slot s decodes frame idx[s], and a
// slot at or past the count returns before any other load. An entry outside the batch is skipped, so
// that nothing a wrong list holds can be used as an address.
template <int LOGN, int L, bool INDEXED>
__global__ void __launch_bounds__((64 * Shape<LOGN, L>::WPB)) polar_sc_list_kernel(
    const Ent *__restrict__ tab, const int8_t *__restrict__ llr, u32 batch, u32 K, u32 poly, u32 clen,
    u32 *__restrict__ info, uint8_t *__restrict__ rank_out, const u32 *__restrict__ idx,
    const u32 *__restrict__ idx_count)
{
    typedef Shape<LOGN, L> S;
    constexpr int N = S::N;
    __shared__ u32 lds[S::WPB * S::WAVE_DW];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    size_t frame = (size_t)blockIdx.x * S::WPB + wave;
    if (frame >= batch) return;                      // (wave-uniform; no block-wide barrier anywhere)
    if constexpr (INDEXED) {
        if (frame >= *idx_count) return;
        frame = (size_t)__builtin_amdgcn_readfirstlane(idx[frame]);
        if (frame >= batch) return;
    }

    Wave<LOGN, L> W;
    W.R = lds + wave * S::WAVE_DW;
    W.A = W.R + S::R_DW;
    W.B = W.A + L * S::A_DW;
    W.T = W.B + L * S::B_DW;
    W.lane = lane;
    W.count = 1;
    W.cur = 0;

    // the channel: N int8 -> int16 pairs, four LLRs per lane and step
    const u32 *src = (const u32 *)(llr + frame * (size_t)N);
    for (int q = (int)lane; q < N / 4; q += 64) {
        const u32 v = src[q];
        const int l0 = (int8_t)(v & 0xFFu), l1 = (int8_t)((v >> 8) & 0xFFu);
        const int l2 = (int8_t)((v >> 16) & 0xFFu), l3 = (int8_t)(v >> 24);
        W.R[2 * q] = ((u32)l0 & 0xFFFFu) | ((u32)l1 << 16);
        W.R[2 * q + 1] = ((u32)l2 & 0xFFFFu) | ((u32)l3 << 16);
    }
    if (lane < (u32)S::T_DW) W.T[lane] = 0u;         // rank 0: metric 0, every level in array 0
    wave_phase();

    u32 mword = 0;
    for (u32 i = 0; i < (u32)N; i++) {
        if (!(i & 31u)) mword = tab[i >> 5].m;       // (uniform: a scalar load)
        if (i == 0u) {
            for (int s = LOGN - 1; s >= 1; s--) W.template node<false>(s);
        } else if (!(i & 1u)) {
            const int t = __builtin_ctz(i);
            W.template node<true>(t);
            for (int s = t - 1; s >= 1; s--) W.template node<false>(s);
        }
        if ((mword >> (i & 31u)) & 1u) W.info_leaf(i);
        else W.frozen_leaf(i);
        W.fold_bits(i);
    }

    // every path's codeword estimate sits in level LOGN of its own partial-sum array
    constexpr int D = S::D, IROW = S::IROW;
    const int count = W.count;
    u32 *img = W.A;                                  // (the LLR arrays are dead)
    for (int x = (int)lane; x < L * IROW; x += 64) img[x] = 0u;
    for (int x = (int)lane; x < count * D; x += 64) {
        u32 *p = W.B + (x / D) * S::B_DW + boff(LOGN) + (x % D);
        *p = xf_dword(*p);
    }
    wave_phase();
    for (int h = 1; h < D; h <<= 1) {                // the stages between dwords
        for (int x = (int)lane; x < count * D; x += 64) {
            const int d = x % D;
            u32 *p = W.B + (x / D) * S::B_DW + boff(LOGN) + d;
            if (!(d & h)) *p ^= p[h];
        }
        wave_phase();
    }
    for (int x = (int)lane; x < count * D; x += 64) {
        const int j = x / D, d = x % D;
        const Ent e = load_ent(tab, (u32)d);
        const u32 c = compress(W.B[j * S::B_DW + boff(LOGN) + d], e);
        u32 *row = img + j * IROW;
        const u32 sh = e.off & 31u, q = e.off >> 5;
        if (e.pc) atomicOr(&row[q], c << sh);
        if (sh + e.pc > 32u) atomicOr(&row[q + 1u], c >> (32u - sh));
    }
    wave_phase();

    bool pass = false;
    if (clen && (int)lane < count) pass = crc_passes(img + lane * IROW, K, poly, clen);
    const unsigned long long votes = __ballot(pass);
    const u32 pick = votes ? (u32)__builtin_ctzll(votes) : 0u;
    const u32 irow = 2u * ((K + 63u) / 64u);
    if (lane < irow) info[frame * irow + lane] = img[pick * IROW + lane];
    if (rank_out && lane == 0u) rank_out[frame] = (uint8_t)((clen && !votes) ? 0xFFu : pick);
}

// idx == nullptr: the direct kernel over frames 0 .. batch - 1; else the indexed kernel
template <int LOGN, int L>
void launch(hipStream_t s, const Ent *tab, const int8_t *llr, u32 batch, u32 K, u32 poly, u32 clen, u32 *info,
            uint8_t *rank_out, const u32 *idx, const u32 *count)
{
    constexpr int WPB = Shape<LOGN, L>::WPB;
    const dim3 blocks((unsigned)(((size_t)batch + WPB - 1) / WPB)), threads(64 * WPB);
    if (idx)
        hipLaunchKernelGGL((polar_sc_list_kernel<LOGN, L, true>), blocks, threads, 0, s, tab, llr, batch, K, poly, clen,
                           info, rank_out, idx, count);
    else
        hipLaunchKernelGGL((polar_sc_list_kernel<LOGN, L, false>), blocks, threads, 0, s, tab, llr, batch, K, poly, clen,
                           info, rank_out, idx, count);
}

template <int LOGN>
void launch_l(int L, hipStream_t s, const Ent *tab, const int8_t *llr, u32 batch, u32 K, u32 poly, u32 clen,
              u32 *info, uint8_t *rank_out, const u32 *idx, const u32 *count)
{
    switch (L) {
    case 1: launch<LOGN, 1>(s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 2: launch<LOGN, 2>(s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 4: launch<LOGN, 4>(s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    default: launch<LOGN, 8>(s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    }
}

void launch_n(uint32_t N, int L, hipStream_t s, const Ent *tab, const int8_t *llr, u32 batch, u32 K, u32 poly,
              u32 clen, u32 *info, uint8_t *rank_out, const u32 *idx, const u32 *count)
{
    switch (N) {
    case 32: launch_l<5>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 64: launch_l<6>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 128: launch_l<7>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 256: launch_l<8>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    case 512: launch_l<9>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    default: launch_l<10>(L, s, tab, llr, batch, K, poly, clen, info, rank_out, idx, count); break;
    }
}

}  // namespace polar_list

// tab_dev: the plan's transform table (polar_sc_xform_table). 32 <= N <= 1024 a power of two,
// L in {1, 2, 4, 8}, 1 <= K <= N, clen = 0 (no CRC) or 1 <= clen <= 32 and < K, 1 <= batch <= 2^31 - 8.
// Returns 0 or a hipError_t.
extern "C" int polar_sc_launch_list(const void *tab_dev, const int8_t *llr_dev, size_t batch, uint32_t N, uint32_t K,
                                    int L, uint32_t poly, uint32_t clen, uint64_t *info_dev, uint8_t *rank_dev,
                                    void *stream)
{
    polar_list::launch_n(N, L, (hipStream_t)stream, (const polar_list::Ent *)tab_dev, llr_dev, (uint32_t)batch, K, poly,
                         clen, (uint32_t *)info_dev, rank_dev, nullptr, nullptr);
    return (int)hipGetLastError();
}

// The same decoder over the frames idx_dev[0 .. *count_dev) only (both written earlier on `stream`;
// idx_dev holds `batch` entries): info_dev and rank_dev rows of the other frames are left alone.
extern "C" int polar_sc_launch_list_indexed(const void *tab_dev, const int8_t *llr_dev, size_t batch, uint32_t N,
                                            uint32_t K, int L, uint32_t poly, uint32_t clen, uint64_t *info_dev,
                                            uint8_t *rank_dev, const uint32_t *idx_dev, const uint32_t *count_dev,
                                            void *stream)
{
    polar_list::launch_n(N, L, (hipStream_t)stream, (const polar_list::Ent *)tab_dev, llr_dev, (uint32_t)batch, K, poly,
                         clen, (uint32_t *)info_dev, rank_dev, idx_dev, count_dev);
    return (int)hipGetLastError();
}

// static LDS per block and waves per block of the kernel for (N, L): the accounting of DESIGN.md 3.11
extern "C" void polar_sc_list_shape(uint32_t N, int L, uint32_t *lds_bytes_per_wave, uint32_t *waves_per_block)
{
    using namespace polar_list;
    int logn = 5;
    while ((1u << logn) < N) logn++;
    uint32_t dw = 0, wpb = 0;
#define POLAR_LIST_CASE(LN, LL) \
    if (logn == LN && L == LL) dw = Shape<LN, LL>::WAVE_DW, wpb = Shape<LN, LL>::WPB;
#define POLAR_LIST_ROW(LN) POLAR_LIST_CASE(LN, 1) POLAR_LIST_CASE(LN, 2) POLAR_LIST_CASE(LN, 4) POLAR_LIST_CASE(LN, 8)
    POLAR_LIST_ROW(5) POLAR_LIST_ROW(6) POLAR_LIST_ROW(7) POLAR_LIST_ROW(8) POLAR_LIST_ROW(9) POLAR_LIST_ROW(10)
#undef POLAR_LIST_ROW
#undef POLAR_LIST_CASE
    *lds_bytes_per_wave = dw * 4u;
    *waves_per_block = wpb;
}
