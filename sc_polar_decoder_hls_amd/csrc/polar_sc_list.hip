// polar_sc_list.hip -- successive-cancellation list decoding (gfx950): the L best paths of the SC
// tree (L = 1 .. 32), ranked by an integer path metric, with an optional CRC inside the payload
// choosing the survivor; int8 LLRs in, information words out, one launch. DESIGN.md 3.11 defines the
// decoding rule; this file follows it bit for bit.
//
// One wave decodes one frame; waves never synchronise with each other. All state of a frame lives
// in the wave's share of LDS:
//   R        the channel LLRs as int16 (level LOGN of the tree, shared by every path)
//   A[p][s]  LLR arrays: level s (a node of 2^s LLRs) of physical array p, int16, at element 2^s
//   B[p][s]  partial sums of the completed left child at level s of physical array p, bit-packed
//   T        per rank: path metric, the two index words below, the bit decided last (PRECODED: with
//            the path's precoder history in the same dword); in two copies
// Paths share arrays through two index words per rank, a field per level: word `a` names the
// physical array that holds the path's LLRs of each level, word `b` the same for the partial sums.
// Every live path walks the tree in lockstep, so a level is rewritten by all paths at once: what
// the level held before is dead for every path, and rank j simply takes physical array j for it.
// A fork therefore copies two index words and nothing else; no level is ever copied, no
// reference is counted, no array is allocated.
//
// The walk is bit by bit (no node shortcuts). Leaf i first recomputes the levels below the lowest
// set bit t of i: G of level t from the parent's arrays (wherever the index word says they are),
// then F down to level 1, packed two int16 per lane; the leaf LLR itself is F or G of the level-1
// pair, taken in a register. An information leaf ranks its 2 * paths <= 64 candidates, candidate
// 2 r + bit in lane 2 r + bit, by the key PM' << (field bits + 1) | r << 1 | bit. Keys are unique;
// the number of smaller keys, counted over 2 L lanes read one by one, is the destination rank, and
// the survivors' state is scattered to their new ranks. Then the decided bits are folded into the
// partial sums: beta = (left ^ right, right) level by level up to the first level that is a left
// child, where it is stored. After the last leaf that is the level-LOGN array: the codeword
// estimate of every path, from which the information words come as in polar_sc_xform.hip
// (transform, compress by the mask with the plan's per-dword table, OR into an LDS image).
//
// Two layouts of that state, chosen from L at compile time (Narrow and Wide below). L <= 8: 32-bit
// index words of 3-bit fields, every LLR level 1 .. LOGN-1 stored. L = 16 and 32 do not fit those
// fields, that key or that LDS budget: 64-bit index words of 5-bit fields (50 bits at N = 1024), and
// level LOGN-1 of the LLRs is never stored. It would be half of every array, and only the level
// below reads it, at four leaves of a frame (0, N/4, N/2, 3N/4): those steps compute their input
// pairs in registers from R. For leaves below N/2 the level is F(R[e], R[e + N/2]), the same for
// every path; from N/2 on it is G(R[e], R[e + N/2], beta) with beta the path's level-(LOGN-1)
// partial sums, found through index word b.
//
// PRECODED ("Precoded codes"): the code has a convolutional precoder ahead of the
// polar transform, u_i = v_i ^ feed_i with feed_i a parity over the path's last conv_len - 1 values of
// v. The tree, the metric and the partial sums work on u as before; a frozen leaf decides u = feed
// (v = 0), an information leaf forks on v. The history h rides in the dword of T that holds the
// decided bit: bits 0 .. 30 = h (bit j - 1 = v_{i-j}), bit 31 = the u decided last. The epilogue turns
// each path's u into v before the compress by the mask.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "polar_sc_xf.h"

namespace polar_list {

using polar_xf::compress;
using polar_xf::Ent;
using polar_xf::load_ent;
using polar_xf::u32;
using polar_xf::wave_phase;
using polar_xf::xf_dword;
typedef unsigned long long u64;
typedef short s16x2 __attribute__((ext_vector_type(2)));

constexpr int GMAX = 32767;     // |G| bound of the rule

// dword of level s inside a path's partial-sum array: levels 0..4 take a dword each, level
// s >= 5 takes 2^(s-5)
__host__ __device__ constexpr int boff(int s) { return s < 5 ? s : 4 + (1 << (s - 5)); }

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

// ---- the two layouts: what the list size forces, and the node steps that differ in substance.
// W is the Wave below; every function is called by the whole wave. -----------------------------------

// L <= 8: one dword per index word, T = two copies of {pm, a, b, bit}[L]
template <int LOGN, int L>
struct Narrow {
    typedef u32 Word;
    static constexpr int FB = 3;                      // bits of a field of an index word
    static constexpr int WORD_DW = 1;
    static constexpr int A_DW = (1 << LOGN) / 2;      // per physical array: levels 1 .. LOGN-1 (+ pad)
    static constexpr int TOP_LEVEL = LOGN - 1;        // the highest stored LLR level
    // waves per block: 4 where they fit the 64 KB of a block's static LDS, else 1 (a CU holds
    // 160 KB: single-wave blocks leave the least of it unused)
    static constexpr int wpb(int wave_dw) { return wave_dw * 4 * 4 <= 65536 ? 4 : 1; }
    static_assert(L <= 8, "a 3-bit field names one of L arrays");

    __device__ __forceinline__ static Word load(const u32 *t, u32 r) { return t[r]; }
    __device__ __forceinline__ static void store(u32 *t, u32 r, Word w) { t[r] = w; }

    // level s (1 <= s < LOGN) of every live path from level s + 1: count * 2^(s-1) LLR pairs over
    // the 64 lanes. F reads the path's own array (written by the step before) or, at the top, the
    // channel; G reads the array the index word names and the partial sums of its left child.
    template <bool IS_G, class W>
    __device__ __forceinline__ static void node(W &w, int s)
    {
        typedef typename W::S S;
        const int sh = s - 1, half = 1 << sh, total = w.count << sh;
        for (int x = (int)w.lane; x < total; x += 64) {
            const int j = x >> sh, e = x & (half - 1);
            const u32 *in;
            u32 u = 0;
            if (s + 1 == LOGN) {
                in = w.R;
            } else {
                const u32 p = IS_G ? W::field(w.word_a(w.cur, j), s + 1) : (u32)j;
                in = w.A + p * S::A_DW + (1 << s);
            }
            if (IS_G) {
                const u32 q = W::field(w.word_b(w.cur, j), s);
                u = w.B[q * S::B_DW + boff(s) + (e >> 4)] >> ((2 * e) & 31);
            }
            const u32 a = in[e], b = in[e + half];
            w.A[j * S::A_DW + half + e] = IS_G ? g_pk(a, b, u) : f_pk(a, b);
        }
        wave_phase();
    }

    // the levels leaf i (even) needs below its lowest set bit, down to level 1
    template <class W>
    __device__ __forceinline__ static void descend(W &w, u32 i)
    {
        if (i == 0u) {
            for (int s = LOGN - 1; s >= 1; s--) node<false>(w, s);
        } else {
            const int t = __builtin_ctz(i);
            node<true>(w, t);
            for (int s = t - 1; s >= 1; s--) node<false>(w, s);
        }
    }
};

// L = 16 or 32: two dwords per index word, T = two copies of {pm, a_lo, a_hi, b_lo, b_hi, bit}[L]
template <int LOGN, int L>
struct Wide {
    typedef u64 Word;
    static constexpr int FB = 5;
    static constexpr int WORD_DW = 2;
    static constexpr int A_DW = (1 << LOGN) / 4;      // per physical array: levels 1 .. LOGN-2 (dword 0 unused)
    static constexpr int TOP_LEVEL = LOGN - 2;
    // waves per block: 4 where four fit the 64 KB of a block's static LDS, else as many as fit
    static constexpr int wpb(int wave_dw) { return 16384 / wave_dw >= 4 ? 4 : 16384 / wave_dw; }
    static_assert(LOGN >= 5 && LOGN <= 10 && (L == 16 || L == 32), "N = 32 .. 1024, 16 or 32 paths");

    __device__ __forceinline__ static Word load(const u32 *t, u32 r) { return (u64)t[r] | ((u64)t[L + r] << 32); }
    __device__ __forceinline__ static void store(u32 *t, u32 r, Word w)
    {
        t[r] = (u32)w;
        t[L + r] = (u32)(w >> 32);
    }

    // how a node step gets level s + 1: from the arrays, or (s = LOGN - 2) from the channel by F or G
    enum Top { STORED = 0, TOP_F = 1, TOP_G = 2 };

    // LLR pair x (0 <= x < N/4) of the virtual level LOGN - 1 of the path whose word b is ib
    template <int TOPK, class W>
    __device__ __forceinline__ static u32 top_pair(W &w, int x, u64 ib)
    {
        typedef typename W::S S;
        const u32 ra = w.R[x], rb = w.R[x + S::N / 4];
        if (TOPK == TOP_F) return f_pk(ra, rb);
        const u32 q = W::field(ib, LOGN - 1);
        return g_pk(ra, rb, w.B[q * S::B_DW + boff(LOGN - 1) + (x >> 4)] >> ((2 * x) & 31));
    }

    // level s (1 <= s <= LOGN - 2) of every live path from level s + 1: count * 2^(s-1) LLR pairs
    // over the 64 lanes. F reads the path's own array (written by the step before), G the array the
    // index word names and the partial sums of its left child; TOPK != STORED (s = LOGN - 2 only)
    // takes level s + 1 from the channel instead.
    template <bool IS_G, int TOPK, class W>
    __device__ __forceinline__ static void node(W &w, int s)
    {
        typedef typename W::S S;
        const int sh = s - 1, half = 1 << sh, total = w.count << sh;
        for (int x = (int)w.lane; x < total; x += 64) {
            const int j = x >> sh, e = x & (half - 1);
            const u64 ib = (IS_G || TOPK == TOP_G) ? w.word_b(w.cur, j) : 0ull;
            u32 a, b, u = 0;
            if (TOPK == STORED) {
                const u32 p = IS_G ? W::field(w.word_a(w.cur, j), s + 1) : (u32)j;
                const u32 *in = w.A + p * S::A_DW + (1 << s);
                a = in[e];
                b = in[e + half];
            } else {
                a = top_pair<TOPK>(w, e, ib);
                b = top_pair<TOPK>(w, e + half, ib);
            }
            if (IS_G) u = w.B[W::field(ib, s) * S::B_DW + boff(s) + (e >> 4)] >> ((2 * e) & 31);
            w.A[j * S::A_DW + half + e] = IS_G ? g_pk(a, b, u) : f_pk(a, b);
        }
        wave_phase();
    }

    // the levels leaf i (even) needs below its lowest set bit, down to level 1
    template <class W>
    __device__ __forceinline__ static void descend(W &w, u32 i)
    {
        typedef typename W::S S;
        int t;
        if (i == 0u) {
            node<false, TOP_F>(w, TOP_LEVEL);
            t = TOP_LEVEL;
        } else {
            t = __builtin_ctz(i);
            if (t == LOGN - 1) {          // i = N/2: G of the virtual level, then F
                node<false, TOP_G>(w, TOP_LEVEL);
                t = TOP_LEVEL;
            } else if (t == TOP_LEVEL) {  // i = N/4 or 3N/4
                if (i < (u32)S::N / 2u) node<true, TOP_F>(w, TOP_LEVEL);
                else node<true, TOP_G>(w, TOP_LEVEL);
            } else {
                node<true, STORED>(w, t);
            }
        }
        for (int s = t - 1; s >= 1; s--) node<false, STORED>(w, s);
    }
};

template <int LOGN, int L>
struct Shape {
    typedef std::conditional_t<(L <= 8), Narrow<LOGN, L>, Wide<LOGN, L>> Lay;
    static constexpr int N = 1 << LOGN;
    static constexpr int D = N / 32;                  // dwords of a codeword
    static constexpr int R_DW = N / 2;                // channel LLRs, int16
    static constexpr int A_DW = Lay::A_DW;
    static constexpr int B_DW = boff(LOGN) + D;       // levels 0 .. LOGN
    static constexpr int T_ROW = 2 + 2 * Lay::WORD_DW;      // dwords per rank: pm, word a, word b, bit
    static constexpr int T_DW = 2 * T_ROW * L;        // two copies
    static constexpr int WAVE_DW = R_DW + L * A_DW + L * B_DW + T_DW;
    static constexpr int WPB = Lay::wpb(WAVE_DW);
    static constexpr int IROW = D < 2 ? 2 : D;        // information-row image per path (dwords), inside A
    static_assert(WPB >= 1, "a wave's state fits a block's static LDS");
    static_assert(IROW <= A_DW, "the information image reuses the LLR arrays");
    static_assert(Lay::FB * LOGN <= 32 * Lay::WORD_DW, "a field per level in an index word");
};

// a 1 in every whole field of an index word
template <class Word, int FB>
__host__ __device__ constexpr Word field_ones()
{
    Word w = 0;
    for (int k = 0; k < (int)(8 * sizeof(Word)) / FB; k++) w |= (Word)1 << (FB * k);
    return w;
}

// The state of one frame; every member function is called by the whole wave.
template <int LOGN, int L, bool PRECODED>
struct Wave {
    typedef Shape<LOGN, L> S;
    typedef typename S::Lay Lay;
    typedef typename Lay::Word Word;
    static constexpr int FB = Lay::FB, ROW = S::T_ROW * L;      // ROW: dwords of a copy of T
    u32 *R, *A, *B, *T;
    u32 lane;
    int count;      // live paths (wave-uniform)
    int cur;        // which copy of T is current
    u32 cmask;      // PRECODED: conv_poly >> 1, the taps on the history (bit j - 1 = c_j)

    static constexpr u32 HMASK = 0x7FFFFFFFu;       // PRECODED: the history bits of a tab_bit dword
    // the u that precoding makes of data bit v on a path whose tab_bit dword is hw
    __device__ __forceinline__ u32 precode(u32 hw, u32 v) const { return v ^ ((u32)__builtin_popcount(hw & cmask) & 1u); }
    // the tab_bit dword after a position that decided data bit v, sent as u
    __device__ __forceinline__ static u32 advance(u32 hw, u32 v, u32 u) { return (u << 31) | ((hw << 1) & HMASK) | v; }

    __device__ __forceinline__ static u32 field(Word w, int s) { return (u32)(w >> (FB * s)) & ((1u << FB) - 1u); }

    __device__ __forceinline__ u32 *tab_pm(int c) { return T + c * ROW; }
    __device__ __forceinline__ u32 *tab_bit(int c) { return T + c * ROW + ROW - L; }
    __device__ __forceinline__ Word word_a(int c, u32 r) { return Lay::load(T + c * ROW + L, r); }
    __device__ __forceinline__ Word word_b(int c, u32 r) { return Lay::load(T + c * ROW + (1 + Lay::WORD_DW) * L, r); }
    __device__ __forceinline__ void set_words(int c, u32 r, Word a, Word b)
    {
        Lay::store(T + c * ROW + L, r, a);
        Lay::store(T + c * ROW + (1 + Lay::WORD_DW) * L, r, b);
    }

    __device__ __forceinline__ void descend(u32 i) { Lay::descend(*this, i); }

    // the LLR of leaf i for path r (r < count): F or G of the level-1 pair
    __device__ __forceinline__ int leaf_llr(u32 i, u32 r)
    {
        if (!(i & 1u)) {
            const u32 v = A[r * S::A_DW + 1];
            return f_one((short)(v & 0xFFFFu), (short)(v >> 16));
        }
        const u32 v = A[field(word_a(cur, r), 1) * S::A_DW + 1];
        const u32 u = B[field(word_b(cur, r), 0) * S::B_DW] & 1u;
        return g_one((short)(v & 0xFFFFu), (short)(v >> 16), u);
    }

    __device__ __forceinline__ void frozen_leaf(u32 i)
    {
        if ((int)lane < count) {
            const int lam = leaf_llr(i, lane);
            if constexpr (PRECODED) {
                const u32 hw = tab_bit(cur)[lane], u = precode(hw, 0u);
                tab_pm(cur)[lane] += u != (u32)(lam < 0) ? (u32)abs(lam) : 0u;
                tab_bit(cur)[lane] = advance(hw, 0u, u);
            } else {
                tab_pm(cur)[lane] += lam < 0 ? (u32)(-lam) : 0u;
                tab_bit(cur)[lane] = 0u;
            }
        }
        wave_phase();
    }

    // candidates 2 r + bit in lanes 0 .. 2 count - 1; the survivors go to the other copy of T. The
    // key keeps r in FB bits (PM' < 2^25, so the key stays below the 0xFFFFFFFF of an idle lane).
    // PRECODED: `bit` is the data bit v, which the key and the history take; the metric judges u.
    __device__ __forceinline__ void info_leaf(u32 i)
    {
        const u32 r = lane >> 1, bit = lane & 1u;
        const bool valid = (int)r < count;
        u32 key = 0xFFFFFFFFu, pm = 0, hw = 0, u = bit;
        Word ia = 0, ib = 0;
        if (valid) {
            const int lam = leaf_llr(i, r);
            ia = word_a(cur, r);
            ib = word_b(cur, r);
            if constexpr (PRECODED) {
                hw = tab_bit(cur)[r];
                u = precode(hw, bit);
            }
            pm = tab_pm(cur)[r] + (u != (u32)(lam < 0) ? (u32)abs(lam) : 0u);
            key = (pm << (FB + 1)) | (r << 1) | bit;
        }
        u32 dest = 0;
#pragma unroll
        for (int k = 0; k < 2 * L; k++) dest += (u32)__builtin_amdgcn_readlane((int)key, k) < key ? 1u : 0u;
        const int nxt = cur ^ 1;
        if (valid && dest < (u32)L) {
            tab_pm(nxt)[dest] = pm;
            set_words(nxt, dest, ia, ib);
            tab_bit(nxt)[dest] = PRECODED ? advance(hw, bit, u) : bit;
        }
        cur = nxt;
        count = min(L, 2 * count);
        wave_phase();
    }

    // fold the bit decided at leaf i into the partial sums: t = the level of the first ancestor that
    // is a left child (LOGN after the last leaf). Levels below 5 fold in a register of lane j =
    // rank j; higher ones in place in the destination, one dword per lane. Then rank j owns array j
    // for that level of the partial sums and for the stored LLR levels among 1 .. t, which the next
    // leaf rewrites.
    __device__ __forceinline__ void fold_bits(u32 i)
    {
        const int t = (i + 1u == (u32)S::N) ? LOGN : __builtin_ctz(i + 1u);
        const bool live = (int)lane < count;
        Word ib = 0;
        if (live) {
            ib = word_b(cur, lane);
            u32 beta = PRECODED ? tab_bit(cur)[lane] >> 31 : tab_bit(cur)[lane];
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
                dst[d] = c ^ B[field(word_b(cur, j), s) * S::B_DW + boff(s) + d];
                dst[w + d] = c;
            }
            wave_phase();
        }
        if (live && t < LOGN) {
            constexpr Word ONE = 1, FM = (ONE << FB) - ONE;             // FM: one field
            const int ta = t < Lay::TOP_LEVEL ? t : Lay::TOP_LEVEL;
            const Word am = ((ONE << (FB * ta + FB)) - ONE) & ~FM;      // fields 1 .. ta
            const Word ia = word_a(cur, lane);
            set_words(cur, lane, (ia & ~am) | (((Word)lane * field_ones<Word, FB>()) & am),
                      (ib & ~(FM << (FB * t))) | ((Word)lane << (FB * t)));
        }
        wave_phase();
    }
};

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
// PRECODED: the code is precoded with the taps cmask = conv_poly >> 1 (0: the identity); direct only.
template <int LOGN, int L, bool INDEXED, bool PRECODED>
__global__ void __launch_bounds__((64 * Shape<LOGN, L>::WPB)) polar_sc_list_kernel(
    const Ent *__restrict__ tab, const int8_t *__restrict__ llr, u32 batch, u32 K, u32 poly, u32 clen,
    u32 *__restrict__ info, uint8_t *__restrict__ rank_out, const u32 *__restrict__ idx,
    const u32 *__restrict__ idx_count, u32 cmask)
{
    static_assert(!(INDEXED && PRECODED), "adaptive decoding has no precoded form");
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

    Wave<LOGN, L, PRECODED> W;
    W.cmask = cmask;
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
    // rank 0: metric 0, every level in array 0
    for (int x = (int)lane; x < S::T_DW; x += 64) W.T[x] = 0u;
    wave_phase();

    u32 mword = 0;
    for (u32 i = 0; i < (u32)N; i++) {
        if (!(i & 31u)) mword = tab[i >> 5].m;       // (uniform: a scalar load)
        if (!(i & 1u)) W.descend(i);
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
    if constexpr (PRECODED) {
        // that array is the path's u: v_i = u_i ^ feed_i, where feed_i needs the v before it. One lane
        // per path, bit-serial through the row with the leaves' own history register.
        if ((int)lane < count) {
            u32 *row = W.B + lane * S::B_DW + boff(LOGN);
            u32 hw = 0;
            for (int d = 0; d < D; d++) {
                const u32 uw = row[d];
                u32 vw = 0;
#pragma unroll
                for (int k = 0; k < 32; k++) {
                    const u32 v = W.precode(hw, (uw >> k) & 1u);    // (the XOR with feed is its own inverse)
                    hw = (hw << 1) | v;     // (bit 31 is no tap)
                    vw |= v << k;
                }
                row[d] = vw;
            }
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
        hipLaunchKernelGGL((polar_sc_list_kernel<LOGN, L, true, false>), blocks, threads, 0, s, tab, llr, batch, K, poly,
                           clen, info, rank_out, idx, count, 0u);
    else
        hipLaunchKernelGGL((polar_sc_list_kernel<LOGN, L, false, false>), blocks, threads, 0, s, tab, llr, batch, K, poly,
                           clen, info, rank_out, idx, count, 0u);
}

// the direct kernel of a code precoded with the taps cmask
template <int LOGN, int L>
void launch_precoded(hipStream_t s, const Ent *tab, const int8_t *llr, u32 batch, u32 K, u32 poly, u32 clen, u32 *info,
                     uint8_t *rank_out, u32 cmask)
{
    constexpr int WPB = Shape<LOGN, L>::WPB;
    const dim3 blocks((unsigned)(((size_t)batch + WPB - 1) / WPB)), threads(64 * WPB);
    hipLaunchKernelGGL((polar_sc_list_kernel<LOGN, L, false, true>), blocks, threads, 0, s, tab, llr, batch, K, poly, clen,
                       info, rank_out, (const u32 *)nullptr, (const u32 *)nullptr, cmask);
}

// one instantiation: its launchers and the LDS accounting of DESIGN.md 3.11 (the same for both)
struct Inst {
    decltype(&launch<5, 1>) launch;
    decltype(&launch_precoded<5, 1>) launch_precoded;
    uint32_t wave_dw, wpb;
};

template <int LOGN, int L>
constexpr Inst inst()
{
    return {launch<LOGN, L>, launch_precoded<LOGN, L>, Shape<LOGN, L>::WAVE_DW, Shape<LOGN, L>::WPB};
}

#define POLAR_LIST_ROW(LN) {inst<LN, 1>(), inst<LN, 2>(), inst<LN, 4>(), inst<LN, 8>(), inst<LN, 16>(), inst<LN, 32>()}
const Inst INST[6][6] = {POLAR_LIST_ROW(5), POLAR_LIST_ROW(6), POLAR_LIST_ROW(7),
                         POLAR_LIST_ROW(8), POLAR_LIST_ROW(9), POLAR_LIST_ROW(10)};
#undef POLAR_LIST_ROW

// the instantiation for N = 2^logn and L paths; null when there is none
const Inst *find(int logn, int L)
{
    if (logn < 5 || logn > 10 || L < 1 || L > 32 || (L & (L - 1))) return nullptr;
    return &INST[logn - 5][__builtin_ctz((unsigned)L)];
}

// log2 N of a power of two, else -1
int log2_exact(uint32_t N) { return (N && !(N & (N - 1u))) ? __builtin_ctz(N) : -1; }

void shape_of(const Inst *k, uint32_t *lds_bytes_per_wave, uint32_t *waves_per_block)
{
    *lds_bytes_per_wave = k ? k->wave_dw * 4u : 0u;
    *waves_per_block = k ? k->wpb : 0u;
}

}  // namespace polar_list

// tab_dev: the plan's transform table (polar_sc_xform_table). 32 <= N <= 1024 a power of two,
// L in {1, 2, 4, 8, 16, 32}, 1 <= K <= N, clen = 0 (no CRC) or 1 <= clen <= 32 and < K,
// 1 <= batch <= 2^31 - 8. idx_dev == NULL: every frame of the batch. Else only the frames
// idx_dev[0 .. *count_dev) (both written earlier on `stream`; idx_dev holds `batch` entries): the
// info_dev and rank_dev rows of the other frames are left alone. Returns 0 or a hipError_t.
extern "C" int polar_sc_launch_list(const void *tab_dev, const int8_t *llr_dev, size_t batch, uint32_t N, uint32_t K,
                                    int L, uint32_t poly, uint32_t clen, uint64_t *info_dev, uint8_t *rank_dev,
                                    const uint32_t *idx_dev, const uint32_t *count_dev, void *stream)
{
    const polar_list::Inst *k = polar_list::find(polar_list::log2_exact(N), L);
    if (!k) return (int)hipErrorInvalidValue;
    k->launch((hipStream_t)stream, (const polar_list::Ent *)tab_dev, llr_dev, (uint32_t)batch, K, poly, clen,
              (uint32_t *)info_dev, rank_dev, idx_dev, count_dev);
    return (int)hipGetLastError();
}

// The direct launch for a precoded code: conv_poly bit j = c_j, c_0 = 1 (judged by the
// caller), so the taps on the history are conv_poly >> 1. Everything else as polar_sc_launch_list.
extern "C" int polar_sc_launch_list_precoded(const void *tab_dev, const int8_t *llr_dev, size_t batch, uint32_t N,
                                             uint32_t K, int L, uint32_t conv_poly, uint32_t poly, uint32_t clen,
                                             uint64_t *info_dev, uint8_t *rank_dev, void *stream)
{
    const polar_list::Inst *k = polar_list::find(polar_list::log2_exact(N), L);
    if (!k) return (int)hipErrorInvalidValue;
    k->launch_precoded((hipStream_t)stream, (const polar_list::Ent *)tab_dev, llr_dev, (uint32_t)batch, K, poly, clen,
                       (uint32_t *)info_dev, rank_dev, conv_poly >> 1);
    return (int)hipGetLastError();
}

// static LDS per wave and waves per block of the kernel for (N, L), L <= 8 (zeros otherwise): the
// accounting of DESIGN.md 3.11
extern "C" void polar_sc_list_shape(uint32_t N, int L, uint32_t *lds_bytes_per_wave, uint32_t *waves_per_block)
{
    int logn = 5;
    while (logn <= 10 && (1u << logn) < N) logn++;
    polar_list::shape_of(L <= 8 ? polar_list::find(logn, L) : nullptr, lds_bytes_per_wave, waves_per_block);
}

// the same for N = 32 .. 1024 a power of two and L = 16 or 32 (zeros otherwise)
extern "C" void polar_sc_list_wide_shape(uint32_t N, int L, uint32_t *lds_bytes_per_wave, uint32_t *waves_per_block)
{
    polar_list::shape_of(L >= 16 ? polar_list::find(polar_list::log2_exact(N), L) : nullptr, lds_bytes_per_wave,
                         waves_per_block);
}
