// polar_sc_scan.hip -- soft-output decoding (gfx950): SCAN, soft cancellation on the SC tree, for
// N = 32 .. 1024. int8 LLRs in; per codeword bit an extrinsic int16 LLR out, and optionally the hard
// codeword row; one launch for 1 .. 8 iterations. DESIGN.md 3.13 defines the rule; this file follows
// it value for value.
//
// One wave decodes one frame; waves never synchronise with each other. A frame's state in the wave's
// share of LDS, all int16:
//   R        the channel (level LOGN of the tree), N values
//   BETA     the beta of every completed node, in place: the node of level s at position p owns
//            BETA[p .. p + 2^s); its children return into the two halves and the node combines them
//            where they lie. After an iteration BETA is the root's beta: the extrinsic output.
//   A[s]     the alpha of the node of level s on the current path, s = TOP .. LOGN - 1 (2^s values)
//   KEPT[s]  (iterations > 1 only) the beta_R every node of level s last received, N/2 values per
//            level, node p's at p/2: what the next iteration's left step reads. Zero at the start.
//
// The walk is by position and depends on the mask alone, so it is the same for every wave. At
// position i (aligned to 2^tt) it takes the largest aligned block [i, i + 2^t), t <= tt, whose
// positions are all frozen or all information: such a subtree returns beta = INF or 0 everywhere
// whatever its alpha and is never entered. The nodes above it that start at i (levels tt .. t + 1) get
// their alpha: level tt by the right step of its parent, the ones below by left steps. Then the block's
// constant is written, and every node that this completes (the block was its right child) combines.
//
// Levels above TOP = min(LOGN, 6) work in LDS, two int16 per lane with the packed 16-bit instructions.
// A node of <= 64 values lives in registers, one value per lane in lane = position mod 64: level s
// keeps each lane's (a, b) pair, reaches its partner lane ^ 2^(s-1) by DPP, ds_swizzle or
// v_permlane32_swap, and both lanes of a pair compute the same step; lanes outside the node compute
// values nobody reads. beta is one register, rewritten only inside the completed node; the kept
// beta_R of levels 1 .. TOP are registers, loaded when a 64-value subtree is entered and stored when
// it returns. Only that entry and that return touch LDS.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "polar_sc_xf.h"

namespace polar_scan {

using polar_xf::Ent;
using polar_xf::u32;
using polar_xf::wave_phase;
typedef unsigned long long u64;
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16;

constexpr int INF = 32767;      // "this bit is 0"
constexpr int LIM = 32766;      // the largest finite magnitude

// f(std::integral_constant<int, HI>) ... f(<LO>), descending; and ascending
template <int LO, int HI, class F>
__device__ __forceinline__ void for_down(F &&f)
{
    if constexpr (HI >= LO) {
        f(std::integral_constant<int, HI>{});
        for_down<LO, HI - 1>(f);
    }
}
template <int LO, int HI, class F>
__device__ __forceinline__ void for_up(F &&f)
{
    if constexpr (LO <= HI) {
        f(std::integral_constant<int, LO>{});
        for_up<LO + 1, HI>(f);
    }
}

// ---- two values per lane ----------------------------------------------------------------------------
__device__ __forceinline__ s16x2 as_pk(u32 x) { return __builtin_bit_cast(s16x2, x); }
__device__ __forceinline__ u32 as_u(s16x2 x) { return __builtin_bit_cast(u32, x); }
// (no operand is ever -32768: the channel is int8, everything else stays inside +-32767)
__device__ __forceinline__ s16x2 pk_abs(s16x2 v) { return __builtin_elementwise_max(v, -v); }

// sign(x) sign(y) min(|x|, |y|); INF is the ordinary value 32767
__device__ __forceinline__ u32 f_pk(u32 x, u32 y)
{
    const s16x2 vx = as_pk(x), vy = as_pk(y);
    const s16x2 m = __builtin_elementwise_min(pk_abs(vx), pk_abs(vy));
    const s16x2 sg = (vx ^ vy) >> 15;
    return as_u((m ^ sg) - sg);
}

// x [+] y, both finite: the saturating packed add, then the clamp to +-32766
__device__ __forceinline__ s16x2 add_pk(u32 x, u32 y)
{
    const s16x2 lo = {-LIM, -LIM}, hi = {LIM, LIM};
    const s16x2 s = __builtin_elementwise_add_sat(as_pk(x), as_pk(y));
    return __builtin_elementwise_min(__builtin_elementwise_max(s, lo), hi);
}
__device__ __forceinline__ u32 box_pk(u32 x, u32 y) { return as_u(add_pk(x, y)); }

// x [+] r, x finite, r a beta_R that may be INF: a 0 / 1 flag from max(r, 32766) - 32766 becomes a
// floor of -32768 / 32767 under the clamped sum
__device__ __forceinline__ u32 box_inf_pk(u32 x, u32 r)
{
    const s16x2 lim = {LIM, LIM}, zero = {0, 0}, top = {(short)-32768, (short)-32768};
    const s16x2 flag = __builtin_elementwise_max(as_pk(r), lim) - lim;
    const s16x2 floor = (zero - flag) ^ top;
    return as_u(__builtin_elementwise_max(add_pk(x, r), floor));
}

// ---- one value per lane -----------------------------------------------------------------------------
__device__ __forceinline__ int f_one(int x, int y)
{
    const int m = min(abs(x), abs(y));
    return ((x ^ y) < 0) ? -m : m;
}
__device__ __forceinline__ int box_one(int x, int y) { return min(max(x + y, -LIM), LIM); }   // (one v_med3_i32)
__device__ __forceinline__ int box_inf_one(int x, int r) { return r == INF ? INF : box_one(x, r); }

// the value of lane ^ H
template <int H>
__device__ __forceinline__ int xchg(int v, u32 lane)
{
    if constexpr (H == 1) {
        return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true);       // quad_perm [1, 0, 3, 2]
    } else if constexpr (H == 2) {
        return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true);       // quad_perm [2, 3, 0, 1]
    } else if constexpr (H == 8) {
        return __builtin_amdgcn_mov_dpp(v, 0x128, 0xF, 0xF, true);      // row_ror:8 (rows of 16 lanes)
    } else if constexpr (H == 32) {
        // the two results: {low half of v in both halves, high half of v in both halves}
        const auto r = __builtin_amdgcn_permlane32_swap((u32)v, (u32)v, false, false);
        return (int)(lane & 32u ? r[0] : r[1]);
    } else {
        return __builtin_amdgcn_ds_swizzle(v, (H << 10) | 0x1F);        // bit mode: and 0x1F, or 0, xor H
    }
}

template <int LOGN, bool KEEP>
struct Shape {
    static constexpr int N = 1 << LOGN;
    static constexpr int TOP = LOGN < 6 ? LOGN : 6;       // the highest level held in registers
    static constexpr int R_DW = N / 2, BETA_DW = N / 2;
    static constexpr int A_DW = (N - (1 << TOP)) / 2;     // levels TOP .. LOGN - 1
    static constexpr int KEPT_LEVEL_DW = N / 4;
    static constexpr int KEPT_DW = KEEP ? LOGN * KEPT_LEVEL_DW : 0;
    static constexpr int WAVE_DW = R_DW + BETA_DW + A_DW + KEPT_DW;
    static constexpr int WPB = 4;
    static_assert(WPB * WAVE_DW * 4 <= 65536, "four waves' state fits a block's static LDS");
    // dword of level s (TOP <= s < LOGN) inside A
    static constexpr int aoff(int s) { return ((1 << s) - (1 << TOP)) / 2; }
};

// The state of one frame; every member function is called by the whole wave.
template <int LOGN, bool KEEP>
struct Wave {
    typedef Shape<LOGN, KEEP> S;
    static constexpr int N = S::N, TOP = S::TOP;
    u32 *R, *BETA, *A, *KEPT;
    u32 lane;
    u32 lm;                 // lane inside the frame (N = 32: lanes 32 .. 63 shadow 0 .. 31 and store nothing)
    int pa[TOP + 1], pb[TOP + 1];   // level s in registers: the lane's pair (alpha[i], alpha[i + 2^(s-1)])
    int kr[TOP + 1];                // the kept beta_R of the lane's node of level s
    int beta;                       // the beta of the lane's position

    __device__ __forceinline__ u32 *kept(int s) { return KEPT + (s - 1) * S::KEPT_LEVEL_DW; }
    __device__ __forceinline__ const u32 *alpha(int s) { return s == LOGN ? R : A + S::aoff(s); }

    // ---- LDS levels: node of level SL > TOP at position p, 2^(SL-2) dwords per half ------------------
    // LEFT: alpha of the left child from the kept beta_R; else of the right child from BETA's left half
    template <int SL, bool LEFT>
    __device__ __forceinline__ void lds_down(u32 p)
    {
        constexpr int H2 = 1 << (SL - 2);
        const u32 *in = alpha(SL);
        u32 *out = A + S::aoff(SL - 1);
        for (int x = (int)lane; x < H2; x += 64) {
            const u32 a = in[x], b = in[H2 + x];
            if (LEFT) out[x] = f_pk(a, KEEP ? box_inf_pk(b, kept(SL)[(p >> 2) + x]) : b);
            else out[x] = box_pk(b, f_pk(a, BETA[(p >> 1) + x]));
        }
        wave_phase();
    }

    template <int SL>
    __device__ __forceinline__ void lds_up(u32 p)
    {
        constexpr int H2 = 1 << (SL - 2);
        const u32 *in = alpha(SL);
        u32 *bl = BETA + (p >> 1), *br = bl + H2;
        for (int x = (int)lane; x < H2; x += 64) {
            const u32 a = in[x], b = in[H2 + x], l = bl[x], r = br[x];
            bl[x] = f_pk(l, box_inf_pk(b, r));
            br[x] = box_inf_pk(f_pk(l, a), r);
            if (KEEP) kept(SL)[(p >> 2) + x] = r;
        }
        wave_phase();
    }

    // an unentered subtree of level t >= TOP at position p returns the constant c
    __device__ __forceinline__ void lds_const(u32 p, int t, int c)
    {
        const u32 cc = ((u32)c & 0xFFFFu) * 0x10001u;
        for (int x = (int)lane; x < (1 << t) / 2; x += 64) BETA[(p >> 1) + x] = cc;
        wave_phase();
    }

    // ---- register levels ----------------------------------------------------------------------------
    // alpha v of the lane's node of level SL (1 <= SL <= TOP) becomes the node's pairs
    template <int SL>
    __device__ __forceinline__ void set_pair(int v)
    {
        constexpr int H = 1 << (SL - 1);
        const int o = xchg<H>(v, lane);
        const bool hi = (lane & (u32)H) != 0u;
        pa[SL] = hi ? o : v;
        pb[SL] = hi ? v : o;
    }

    // the 2^TOP-value subtree at position p is entered: its alpha from LDS, its kept beta_R
    __device__ __forceinline__ void reg_enter(u32 p)
    {
        const u16 *in = (const u16 *)alpha(TOP);
        set_pair<TOP>((short)in[lm]);
        for_up<1, TOP>([&](auto s_) {
            constexpr int s = decltype(s_)::value, H = 1 << (s - 1);
            const u32 q = p + lm;
            kr[s] = KEEP ? (short)((const u16 *)kept(s))[((q & ~(2u * H - 1u)) >> 1) + (q & (H - 1u))] : 0;
        });
    }

    // ... and has returned: its beta to BETA, the kept beta_R back (both lanes of a pair hold the same)
    __device__ __forceinline__ void reg_leave(u32 p)
    {
        if (lane < (u32)N) {
            ((u16 *)BETA)[p + lane] = (u16)beta;
            if (KEEP)
                for_up<1, TOP>([&](auto s_) {
                    constexpr int s = decltype(s_)::value, H = 1 << (s - 1);
                    const u32 q = p + lane;
                    ((u16 *)kept(s))[((q & ~(2u * H - 1u)) >> 1) + (q & (H - 1u))] = (u16)kr[s];
                });
        }
        wave_phase();
    }

    // node of level SL (2 <= SL <= TOP): the alpha of its left (LEFT) or right child of level SL - 1
    template <int SL, bool LEFT>
    __device__ __forceinline__ void reg_down()
    {
        if (LEFT) set_pair<SL - 1>(f_one(pa[SL], box_inf_one(pb[SL], kr[SL])));
        else set_pair<SL - 1>(box_one(pb[SL], f_one(pa[SL], xchg<(1 << (SL - 1))>(beta, lane))));   // (read in the high lanes)
    }

    // node of level SL (1 <= SL <= TOP) at position p: both children have returned
    template <int SL>
    __device__ __forceinline__ void reg_up(u32 p)
    {
        constexpr int H = 1 << (SL - 1);
        const int o = xchg<H>(beta, lane);
        const bool hi = (lane & (u32)H) != 0u;
        const int l = hi ? o : beta, r = hi ? beta : o;
        const int nb = hi ? box_inf_one(f_one(l, pa[SL]), r) : f_one(l, box_inf_one(pb[SL], r));
        const bool inside = (((lm ^ p) & 63u) >> SL) == 0u;      // (the lane is position mod 64)
        beta = inside ? nb : beta;
        if (KEEP) kr[SL] = inside ? r : kr[SL];
    }
};

template <int LOGN, bool KEEP>
__global__ void __launch_bounds__((64 * Shape<LOGN, KEEP>::WPB)) polar_sc_scan_kernel(
    const Ent *__restrict__ tab, const int8_t *__restrict__ llr, u32 batch, int iterations, u32 *__restrict__ ext,
    u64 *__restrict__ hard)
{
    typedef Shape<LOGN, KEEP> S;
    constexpr int N = S::N, TOP = S::TOP, D = N / 32;
    __shared__ u32 lds[S::WPB * S::WAVE_DW];
    const u32 lane = threadIdx.x & 63u;
    const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t frame = (size_t)blockIdx.x * S::WPB + wave;
    if (frame >= batch) return;                      // (wave-uniform; no block-wide barrier anywhere)

    Wave<LOGN, KEEP> W;
    W.R = lds + wave * S::WAVE_DW;
    W.BETA = W.R + S::R_DW;
    W.A = W.BETA + S::BETA_DW;
    W.KEPT = W.A + S::A_DW;
    W.lane = lane;
    W.lm = lane & (u32)(N - 1);
    W.beta = 0;

    // the mask: dword d in lane d, and which dwords are all frozen / all information
    const u32 mreg = lane < (u32)D ? tab[lane].m : 0u;
    const u32 all0 = (u32)__ballot(lane < (u32)D && mreg == 0u);
    const u32 all1 = (u32)__ballot(lane < (u32)D && mreg == 0xFFFFFFFFu);

    // the channel: N int8 -> int16 pairs, four LLRs per lane and step
    const u32 *src = (const u32 *)(llr + frame * (size_t)N);
    for (int q = (int)lane; q < N / 4; q += 64) {
        const u32 v = src[q];
        const int l0 = (int8_t)(v & 0xFFu), l1 = (int8_t)((v >> 8) & 0xFFu);
        const int l2 = (int8_t)((v >> 16) & 0xFFu), l3 = (int8_t)(v >> 24);
        W.R[2 * q] = ((u32)l0 & 0xFFFFu) | ((u32)l1 << 16);
        W.R[2 * q + 1] = ((u32)l2 & 0xFFFFu) | ((u32)l3 << 16);
    }
    if (KEEP)
        for (int x = (int)lane; x < S::KEPT_DW; x += 64) W.KEPT[x] = 0u;
    wave_phase();

    // 0: the block [i, i + 2^t) is all frozen, 1: all information, 2: neither (i aligned to 2^t)
    auto block_kind = [&](u32 i, int t) -> int {
        if (t <= 5) {
            const u32 w = (u32)__builtin_amdgcn_readlane((int)mreg, (int)(i >> 5));
            const u32 ones = t == 5 ? 0xFFFFFFFFu : (1u << (1u << t)) - 1u;
            const u32 v = (w >> (i & 31u)) & ones;
            return v == 0u ? 0 : v == ones ? 1 : 2;
        }
        const u32 wd = 1u << (t - 5);
        const u32 rm = (wd == 32u ? 0xFFFFFFFFu : (1u << wd) - 1u) << (i >> 5);
        return (all0 & rm) == rm ? 0 : (all1 & rm) == rm ? 1 : 2;
    };

    for (int it = 0; it < iterations; it++) {
        for (u32 i = 0; i < (u32)N;) {
            const int tt = i ? __builtin_ctz(i) : LOGN;
            int t = 0, kind = block_kind(i, 0);
            while (t < tt) {
                const int k = block_kind(i, t + 1);
                if (k == 2) break;
                kind = k;
                t++;
            }
            // alpha of the nodes that start here, levels tt .. t + 1 (the root's is the channel)
            for_down<1, LOGN>([&](auto s_) {
                constexpr int s = decltype(s_)::value;
                if (s <= tt && s > t) {
                    if constexpr (s < LOGN) {
                        if constexpr (s >= TOP) {
                            if (s == tt) W.template lds_down<s + 1, false>(i - (1u << s));
                            else W.template lds_down<s + 1, true>(i);
                        } else {
                            if (s == tt) W.template reg_down<s + 1, false>();
                            else W.template reg_down<s + 1, true>();
                        }
                    }
                    if constexpr (s == TOP) W.reg_enter(i);
                }
            });
            // the block returns its constant
            const int c = kind ? 0 : INF;
            if (t >= TOP) W.lds_const(i, t, c);
            else W.beta = (((W.lm ^ i) & 63u) >> t) == 0u ? c : W.beta;
            // every node this completes: levels t + 1 .. t + (trailing ones of i >> t)
            const int last = t + __builtin_ctz(~(i >> t));
            for_up<1, LOGN>([&](auto s_) {
                constexpr int s = decltype(s_)::value;
                if (s > t && s <= last) {
                    const u32 p = i & ~((1u << s) - 1u);
                    if constexpr (s > TOP) {
                        W.template lds_up<s>(p);
                    } else {
                        W.template reg_up<s>(p);
                        if constexpr (s == TOP) W.reg_leave(p);
                    }
                }
            });
            i += 1u << t;
        }
    }

    // ext: the root's beta, one dword (two values) per lane; x^: the sign of llr [+] ext, a ballot per
    // 64 positions (ext = INF gives a positive sum)
    u32 *erow = ext + frame * (size_t)(N / 2);
    for (int x = (int)lane; x < N / 2; x += 64) erow[x] = W.BETA[x];
    if (hard) {
        u64 word = 0;
        for (int cidx = 0; cidx < (N + 63) / 64; cidx++) {
            const u32 e = (u32)cidx * 64u + lane;
            bool neg = false;
            if (e < (u32)N) neg = (int)(short)((const u16 *)W.R)[e] + (int)(short)((const u16 *)W.BETA)[e] < 0;
            const u64 b = __ballot(neg);
            if (lane == (u32)cidx) word = b;
        }
        if (lane < (u32)((N + 63) / 64)) hard[frame * (size_t)((N + 63) / 64) + lane] = word;
    }
}

template <int LOGN, bool KEEP>
void launch(hipStream_t s, const Ent *tab, const int8_t *llr, u32 batch, int iterations, u32 *ext, u64 *hard)
{
    constexpr int WPB = Shape<LOGN, KEEP>::WPB;
    const dim3 blocks((unsigned)(((size_t)batch + WPB - 1) / WPB)), threads(64 * WPB);
    hipLaunchKernelGGL((polar_sc_scan_kernel<LOGN, KEEP>), blocks, threads, 0, s, tab, llr, batch, iterations, ext, hard);
}

// one instantiation: its launcher and the LDS accounting of DESIGN.md 3.13
struct Inst {
    decltype(&launch<5, false>) launch;
    uint32_t wave_dw, wpb;
};

template <int LOGN, bool KEEP>
constexpr Inst inst()
{
    return {launch<LOGN, KEEP>, Shape<LOGN, KEEP>::WAVE_DW, Shape<LOGN, KEEP>::WPB};
}

#define POLAR_SCAN_ROW(LN) {inst<LN, false>(), inst<LN, true>()}
const Inst INST[6][2] = {POLAR_SCAN_ROW(5), POLAR_SCAN_ROW(6), POLAR_SCAN_ROW(7),
                         POLAR_SCAN_ROW(8), POLAR_SCAN_ROW(9), POLAR_SCAN_ROW(10)};
#undef POLAR_SCAN_ROW

// the instantiation for N and the iteration count (one iteration keeps no beta_R); null when there is none
const Inst *find(uint32_t N, int iterations)
{
    if (N < 32u || N > 1024u || (N & (N - 1u)) || iterations < 1 || iterations > 8) return nullptr;
    return &INST[__builtin_ctz(N) - 5][iterations > 1];
}

}  // namespace polar_scan

// tab_dev: the plan's transform table (polar_sc_xform_table). 32 <= N <= 1024 a power of two,
// 1 <= iterations <= 8, 1 <= batch <= 2^31 - 8, hard_dev may be NULL. Returns 0 or a hipError_t.
extern "C" int polar_sc_launch_scan(const void *tab_dev, const int8_t *llr_dev, size_t batch, uint32_t N, int iterations,
                                    int16_t *ext_dev, uint64_t *hard_dev, void *stream)
{
    const polar_scan::Inst *k = polar_scan::find(N, iterations);
    if (!k) return (int)hipErrorInvalidValue;
    k->launch((hipStream_t)stream, (const polar_scan::Ent *)tab_dev, llr_dev, (uint32_t)batch, iterations,
              (uint32_t *)ext_dev, (polar_scan::u64 *)hard_dev);
    return (int)hipGetLastError();
}

// static LDS per wave and waves per block of the kernel for (N, iterations); zeros when there is none
extern "C" void polar_sc_scan_shape(uint32_t N, int iterations, uint32_t *lds_bytes_per_wave, uint32_t *waves_per_block)
{
    const polar_scan::Inst *k = polar_scan::find(N, iterations);
    *lds_bytes_per_wave = k ? k->wave_dw * 4u : 0u;
    *waves_per_block = k ? k->wpb : 0u;
}
