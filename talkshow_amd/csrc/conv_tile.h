// Pieces shared by the two engines of conv_gemm_f32 (conv_gemm.hip: global -> VGPR -> LDS staging; conv_gemm_ring.hip: LDS-DMA
// ring): the per-problem operand pointers of a tile and the epilogue.  One definition, so that both engines store the same bits.
#pragma once
#include "kernels.h"

namespace ts {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) f32x4 lds_f32x4;   // LDS-qualified: volatile accesses must not fall back to flat

struct ConvTilePtrs {
    const float *x, *w, *bias, *res;
    float *out;
};

// pointers of problem / group `zidx` (batched problems shift every pointer by the problem's offsets)
__device__ __forceinline__ ConvTilePtrs conv_tile_ptrs(const ConvParams &p, const ConvGroup &g, const int zidx) {
    ConvTilePtrs t{g.x, g.w, g.bias, g.res, g.out};
    if (p.zdiv > 0) {
        const int z0 = zidx / p.zdiv, z1 = zidx - z0 * p.zdiv;
        t.x += z0 * p.x_zs0 + z1 * p.x_zs1;
        t.w += z0 * p.w_zs0 + z1 * p.w_zs1;
        t.out += z0 * p.o_zs0 + z1 * p.o_zs1;
        if (t.bias) t.bias += z1 * p.b_zs1;
        if (t.res) t.res += z0 * p.r_zs0 + z1 * p.r_zs1;
    }
    return t;
}

// ---- epilogue: bias (+ residual) + activation, masked store ----
// The MFMA operands are swapped (weights as A, activations as B: the same products in the same k order, the same bits), so an
// accumulator block holds D[channel][row]: lane (li, lh) owns output row m = li and, per group g of 4 registers, the 4
// CONSECUTIVE channels 8 g + 4 lh .. + 3 — bias, residual and output move as 16-byte vectors (4 stores per 32 x 32 block
// instead of 16; the residual values of a block are fetched together, ahead of their use).  Rows / buffers that are not
// 16-byte aligned (the 39- / 90- / 129-wide pose rows) and channel tails take the scalar form.
// (mw, nw): first row / column of this wave's TM x TN blocks of 32 x 32.
// MASK (ConvParams::lens given): rows at or beyond their clip's valid length are stored as zeros.  A variant of its own: the
// unmasked instantiations keep the code they had (no register, no branch added to an epilogue that shows in the profile).
template <int TM, int TN, bool MASK = false>
__device__ __forceinline__ void conv_tile_epilogue(const ConvParams &p, const ConvGroup &g, const ConvTilePtrs &t,
                                                   f32x16 (&acc)[TM][TN], const int mw, const int nw, const int li, const int lh) {
    const float *gbias = t.bias, *gres = t.res;
    float *gout = t.out;
    const bool vec_out = ((p.ldo | g.out_col0) & 3) == 0 && (reinterpret_cast<uintptr_t>(gout) & 15) == 0;
    const bool vec_res = gres && (p.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(gres) & 15) == 0;
    const bool vec_bias = gbias && (reinterpret_cast<uintptr_t>(gbias) & 15) == 0;
    auto activate = [&](float v, float rvv) {
        if (gres && !p.res_after_act) v += rvv;
        if (p.act == 1) v = v >= 0.f ? v : v * 0.2f;
        else if (p.act == 2) v = v > 0.f ? v : 0.f;
        else if (p.act == 3) v = gelu_fast(v);   // kernels.h
        if (gres && p.res_after_act) v += rvv;
        return v;
    };
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = mw + i * 32 + li;
        const bool mok = m < p.M;
        bool live = true;   // MASK: row m lies inside its clip (one division per 32-row block and lane, not per stored element)
        if constexpr (MASK) {
            if (mok) {
                const int b = m / p.Lout, t = m - b * p.Lout;
                live = t < ((p.lens[b] >> p.len_shr) << p.len_shl);
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int nb0 = nw + j * 32 + 4 * lh;
            f32x4 rv[4], bv[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int nb = nb0 + 8 * q;
                const bool full = nb + 3 < p.N;
                bv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (gbias) {
                    if (vec_bias && full) bv[q] = *reinterpret_cast<const f32x4 *>(gbias + nb);
                    else
#pragma unroll
                        for (int r = 0; r < 4; ++r) bv[q][r] = nb + r < p.N ? gbias[nb + r] : 0.f;
                }
                rv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (gres && mok) {
                    const float *rp = gres + (long)m * p.ldr + nb;
                    if (vec_res && full) rv[q] = *reinterpret_cast<const f32x4 *>(rp);
                    else
#pragma unroll
                        for (int r = 0; r < 4; ++r) rv[q][r] = nb + r < p.N ? rp[r] : 0.f;
                }
            }
            if (mok) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int nb = nb0 + 8 * q;
                    f32x4 v;
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = activate(acc[i][j][4 * q + r] + bv[q][r], rv[q][r]);
                    if constexpr (MASK) {
                        if (!live) v = f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                    float *op = gout + (long)m * p.ldo + g.out_col0 + nb;
                    if (vec_out && nb + 3 < p.N) *reinterpret_cast<f32x4 *>(op) = v;
                    else
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (nb + r < p.N) op[r] = v[r];
                }
            }
        }
    }
}

// the engines behind launch_conv_plan (conv_gemm.hip), which resolves p.zero and then hands each plan to its launcher
hipError_t launch_conv_gemm_ring(const ConvParams &p, const ConvPlan &plan, hipStream_t stream);   // Ring / RingDealt (conv_gemm_ring.hip)
hipError_t launch_conv_gemm_ring_banded(const ConvParams &p, const ConvBands &bd, hipStream_t stream);
hipError_t launch_conv_gemm_ring_sk(const ConvParams &p, const ConvSK &sk, hipStream_t stream);
bool conv_gemm_ring_takes(const ConvParams &p);   // host: every segment a multiple of the 32-deep stage
// host: the ring engine's plan by tile count: RingDealt with 128 x 128 or 96 x 128 tiles, RingBanded (if `bd` is given) or RingSK (if `sk` is given)
ConvPlan conv_gemm_ring_pick(const ConvParams &p, const ConvBands *bd, const ConvSK *sk);
hipError_t launch_conv_taps48(const ConvParams &p, hipStream_t stream);   // conv_taps48.hip: the wav2vec2 positional convolution
// the same convolution on the bf16 matrix cores with fp32 operands split into `planes` bf16 terms (2: three products, ~2^-16;
// 3: six products, fp32 grade) — conv_gemm_split.hip; an opt-in plan for tolerance-only GEMMs (the face generator)
hipError_t launch_conv_gemm_split(const ConvParams &p, int planes, hipStream_t stream);

}  // namespace ts
