// polar_sc_quant.h -- the reference's sc_quantizer (src/testbench/sc_quantizer/sc_quantizer.h:76-80)
// on the device: q = clamp((short)(v * beta), vsatn, vsatp), for float / half / bfloat16 channel
// values. Shared by the test frame source (polar_sc_channel.hip), the stand-alone quantizer
// (polar_sc_soft.hip) and, as text, the fused per-mask kernel (polar_sc_jit.cpp, Gen::run_mask
// soft mode: pasted into the generated source, so it names no header of its own and no <cstdint>
// type).
#ifndef POLAR_SC_QUANT_H
#define POLAR_SC_QUANT_H

namespace polar_quant {

enum { F32 = 0, F16 = 1, BF16 = 2 };   // POLAR_SC_F32 / F16 / BF16 (include/polar_sc.h)

// (short)(float) of the reference on x86-64: 32-bit truncating conversion (out of range and
// NaN -> 0x80000000), then the low 16 bits. |v| >= 32768 therefore wraps, as the reference does.
__device__ __forceinline__ int to_short(float v)
{
    const int i = (v > -2147483648.0f && v < 2147483648.0f) ? (int)v : (int)0x80000000u;
    return (int)(short)(unsigned short)(unsigned int)i;
}

// one value: a single fp32 multiply, to_short, the clamp as one v_med3_i32 (lo <= hi: the median
// is the clamped value). The multiply is named: one v_mul_f32 per value, with nothing to contract
// it with and not paired by the compiler into a packed fp32 multiply, whatever its flags.
__device__ __forceinline__ int quant(float v, float beta, int lo, int hi)
{
    float m;
    asm("v_mul_f32 %0, %1, %2" : "=v"(m) : "v"(v), "v"(beta));
    const int s = to_short(m);
    int q;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(q) : "v"(s), "v"(lo), "v"(hi));
    return q;
}

template <int DT>
struct elem {
    static constexpr int bytes = DT == F32 ? 4 : 2;
};

// one element at index i of an array of DT (element loads: heads, tails, unaligned inputs)
template <int DT>
__device__ __forceinline__ float load_elem(const void *base, unsigned long i)
{
    if constexpr (DT == F32) {
        return ((const float *)base)[i];
    } else if constexpr (DT == F16) {
        return (float)((const _Float16 *)base)[i];
    } else {
        return __builtin_bit_cast(float, (unsigned int)((const unsigned short *)base)[i] << 16);
    }
}

// E values from the E * bytes / 4 dwords that hold them: fp32 as it is, half by the packed
// convert (exact), bfloat16 by a shift / a mask (exact: it is the high half of the fp32)
template <int DT, int E>
__device__ __forceinline__ void widen(const unsigned int *raw, float *x)
{
    if constexpr (DT == F32) {
#pragma unroll
        for (int i = 0; i < E; i++) x[i] = __builtin_bit_cast(float, raw[i]);
    } else if constexpr (DT == F16) {
        typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
        typedef float f2_t __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int i = 0; i < E / 2; i++) {
            const f2_t w = __builtin_convertvector(__builtin_bit_cast(h2_t, raw[i]), f2_t);
            x[2 * i] = w.x;
            x[2 * i + 1] = w.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < E / 2; i++) {
            x[2 * i] = __builtin_bit_cast(float, raw[i] << 16);
            x[2 * i + 1] = __builtin_bit_cast(float, raw[i] & 0xFFFF0000u);
        }
    }
}

// 16 output bytes of one lane: E = 128 / BITS values (16 int8 or 8 int16) from their raw dwords.
// Four int8 pack with two v_perm_b32 and an OR (selector 0x0C = a zero byte), two int16 with one.
template <int DT, int BITS>
__device__ __forceinline__ uint4 quant_vec(const uint4 *r, float beta, int lo, int hi)
{
    constexpr int E = 128 / BITS, NR = E * elem<DT>::bytes / 16;
    unsigned int raw[4 * NR];
#pragma unroll
    for (int k = 0; k < NR; k++) {
        raw[4 * k] = r[k].x;
        raw[4 * k + 1] = r[k].y;
        raw[4 * k + 2] = r[k].z;
        raw[4 * k + 3] = r[k].w;
    }
    float x[E];
    widen<DT, E>(raw, x);
    unsigned int q[E], o[4];
#pragma unroll
    for (int i = 0; i < E; i++) q[i] = (unsigned int)quant(x[i], beta, lo, hi);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        if constexpr (BITS == 8)
            o[j] = __builtin_amdgcn_perm(q[4 * j + 1], q[4 * j], 0x0C0C0400u) |
                   __builtin_amdgcn_perm(q[4 * j + 3], q[4 * j + 2], 0x04000C0Cu);
        else
            o[j] = __builtin_amdgcn_perm(q[2 * j + 1], q[2 * j], 0x05040100u);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

}  // namespace polar_quant

#endif  // POLAR_SC_QUANT_H
