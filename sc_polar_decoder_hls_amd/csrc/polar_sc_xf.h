// polar_sc_xf.h -- what the kernels that turn a codeword estimate into information words share
// (polar_sc_xform.hip, polar_sc_list.hip, polar_sc_adaptive.hip): the record of the plan's per-dword
// mask table and its bit helpers, and the phase fence of a wave that works alone in LDS.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace polar_xf {

typedef uint32_t u32;

// per-dword record of the plan's table (polar_sc_xform_table): everything the device needs to
// know about the mask, so that it does no mask arithmetic and takes no data-dependent branch
struct __attribute__((aligned(32))) Ent {
    u32 m;       // mask bits of the dword (1 = information)
    u32 off;     // information bits before this dword
    u32 mv[5];   // move masks of the parallel-suffix compress (Hacker's Delight 7-4)
    u32 pc;      // popcount(m)
};

// a record in two 16-byte loads (the table is 32-byte aligned)
__device__ __forceinline__ Ent load_ent(const Ent *__restrict__ tab, size_t d)
{
    const uint4 *q = (const uint4 *)(tab + d);
    const uint4 a = q[0], b = q[1];
    Ent e;
    e.m = a.x; e.off = a.y; e.mv[0] = a.z; e.mv[1] = a.w;
    e.mv[2] = b.x; e.mv[3] = b.y; e.mv[4] = b.z; e.pc = b.w;
    return e;
}

// the bits of x under e.m, packed at the low end in position order
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

// the five stages of u = x F^{(x)n} inside a dword (bit distance 1..16): bit j with the distance
// bit clear takes bit j + h
__device__ __forceinline__ u32 xf_dword(u32 w)
{
    w ^= (w >> 1) & 0x55555555u;
    w ^= (w >> 2) & 0x33333333u;
    w ^= (w >> 4) & 0x0F0F0F0Fu;
    w ^= (w >> 8) & 0x00FF00FFu;
    w ^= (w >> 16) & 0x0000FFFFu;
    return w;
}

// orders the phases of a wave's own LDS state (clear, write, read): LDS executes one wave's
// instructions in order, so only the compiler has to be held
__device__ __forceinline__ void wave_phase()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace polar_xf
