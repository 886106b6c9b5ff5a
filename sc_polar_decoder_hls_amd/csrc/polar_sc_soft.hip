// polar_sc_soft.hip -- the reference's sc_quantizer as a stand-alone kernel (gfx950): float /
// half / bfloat16 channel values -> int8 or int16 LLRs, for any data (polar_sc_quantize) and as
// the front end of polar_sc_decode_soft for every plan whose decode kernel does not quantize
// itself (pair, hybrid and interpreter plans); DESIGN.md 3.9. The per-mask kernel's fused form
// of the same code is generated (polar_sc_jit.cpp, Gen::run_mask); both use polar_sc_quant.h.
//
// Work split: a lane owns 16 output bytes (16 int8 or 8 int16), written by one 16-byte store,
// and reads their 64 / 32 / 16 input bytes with 16-byte loads. The vector body starts at the
// first 16-byte boundary of the OUTPUT; the elements before it (the head) and after the last
// whole vector (the tail), at most 15 each, are done one by one by block 0. An input that is
// not 16-byte aligned at the body's first element is read element by element instead.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "polar_sc_quant.h"

namespace polar_soft {

constexpr int THREADS = 256;
constexpr unsigned MAX_BLOCKS = 8192;   // grid-stride beyond (32 waves per SIMD's worth of blocks)

template <int DT, int BITS>
__device__ __forceinline__ void store_elem(void *q, size_t i, const void *v, float beta, int lo, int hi)
{
    const int x = polar_quant::quant(polar_quant::load_elem<DT>(v, i), beta, lo, hi);
    if constexpr (BITS == 8) ((int8_t *)q)[i] = (int8_t)x;
    else ((int16_t *)q)[i] = (int16_t)x;
}

// head: elements [0, head); body: nvec vectors of E elements from `head`; tail: the rest up to n
template <int DT, int BITS>
__global__ void __launch_bounds__(THREADS) quantize_kernel(const void *__restrict__ v, void *__restrict__ q, size_t n,
                                                           unsigned head, size_t nvec, int in_aligned, float beta,
                                                           int lo, int hi)
{
    constexpr int E = 128 / BITS, ES = polar_quant::elem<DT>::bytes, NR = E * ES / 16;
    const unsigned char *vb = (const unsigned char *)v + (size_t)head * ES;   // body: input
    uint4 *qb = (uint4 *)((unsigned char *)q + (size_t)head * (BITS / 8));    //       output (16-byte aligned)
    const size_t stride = (size_t)gridDim.x * THREADS;
    for (size_t k = (size_t)blockIdx.x * THREADS + threadIdx.x; k < nvec; k += stride) {
        uint4 r[NR];
        if (in_aligned) {
#pragma unroll
            for (int j = 0; j < NR; j++) r[j] = ((const uint4 *)(vb + k * (size_t)(E * ES)))[j];
        } else {   // element loads into the same raw layout
            unsigned int raw[4 * NR];
#pragma unroll
            for (int j = 0; j < 4 * NR; j++) {
                if constexpr (ES == 4) raw[j] = ((const unsigned int *)vb)[k * E + j];
                else raw[j] = (unsigned int)((const unsigned short *)vb)[k * E + 2 * j] |
                              ((unsigned int)((const unsigned short *)vb)[k * E + 2 * j + 1] << 16);
            }
#pragma unroll
            for (int j = 0; j < NR; j++) r[j] = make_uint4(raw[4 * j], raw[4 * j + 1], raw[4 * j + 2], raw[4 * j + 3]);
        }
        qb[k] = polar_quant::quant_vec<DT, BITS>(r, beta, lo, hi);
    }
    if (blockIdx.x == 0) {
        const size_t t = threadIdx.x, tail0 = (size_t)head + nvec * E;
        if (t < head) store_elem<DT, BITS>(q, t, v, beta, lo, hi);
        if (tail0 + t < n) store_elem<DT, BITS>(q, tail0 + t, v, beta, lo, hi);   // (n - tail0 < E <= 16)
    }
}

template <int DT, int BITS>
int launch(const void *v, void *q, size_t n, float beta, int lo, int hi, hipStream_t s)
{
    constexpr int E = 128 / BITS, ES = polar_quant::elem<DT>::bytes, OS = BITS / 8;
    size_t head = ((16u - ((uintptr_t)q & 15u)) & 15u) / OS;   // elements up to the output's 16-byte boundary
    if (head > n) head = n;
    const size_t nvec = (n - head) / E;
    const int in_aligned = (((uintptr_t)v + head * ES) & 15u) == 0u;
    size_t blocks = (nvec + THREADS - 1) / THREADS;
    blocks = blocks < 1 ? 1 : (blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks);
    hipLaunchKernelGGL((quantize_kernel<DT, BITS>), dim3((unsigned)blocks), dim3(THREADS), 0, s, v, q, n, (unsigned)head,
                       nvec, in_aligned, beta, lo, hi);
    return (int)hipGetLastError();
}

}  // namespace polar_soft

// n values of `dtype` (POLAR_SC_F32 / F16 / BF16) at v_dev -> int8 (bits = 8) or int16 (bits = 16)
// at q_dev; both pointers aligned to their element. The arguments are checked by the caller
// (polar_sc_host.cpp). Returns 0 or the hipError_t of the launch.
extern "C" int polar_sc_launch_quantize(const void *v_dev, int dtype, size_t n, int beta, int vsatn, int vsatp,
                                        void *q_dev, int bits, void *stream)
{
    using namespace polar_soft;
    hipStream_t s = (hipStream_t)stream;
    const float b = (float)beta;
    switch (dtype * 2 + (bits == 16)) {
    case 0: return launch<polar_quant::F32, 8>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    case 1: return launch<polar_quant::F32, 16>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    case 2: return launch<polar_quant::F16, 8>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    case 3: return launch<polar_quant::F16, 16>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    case 4: return launch<polar_quant::BF16, 8>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    default: return launch<polar_quant::BF16, 16>(v_dev, q_dev, n, b, vsatn, vsatp, s);
    }
}
