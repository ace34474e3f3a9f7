// VQ codebook search, gathers, the per-position sampler and small glue kernels.
//
//   vq_argmin   VectorQuantizerEMA.get_code_indices   nets/spg/vqvae_modules.py:311-319
//   gather_rows VectorQuantizerEMA.quantize + the (B,W,64)->(B,64,W) permute of VQVAE.decode (a no-op in NLC)
//               nets/spg/vqvae_modules.py:321-323, nets/spg/vqvae_1d.py:201-208
//   sample      softmax + multinomial(1) of GatedPixelCNN.generate, or the greedy argmax harness
//               nets/spg/gated_pixelcnn_v2.py:173-176
#include "kernels.h"
#include "skinny_desc.h"
#include <cstring>
#include "../../include/talkshow_hip.h"

namespace ts {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------------------------
// vq_argmin: one workgroup = ROWS query rows x all codes.  Queries sit in LDS; each thread walks codes
// j = tid, tid+256, ... (ascending, so a strict '<' keeps the lowest index on ties), reading the code row as
// 16-byte loads straight from L2 (the 2048x64 fp32 codebook is 512 KiB and stays cache resident).  Distance is
// evaluated in the reference's association: (|x|^2 + |e_j|^2) - 2*(x.e_j).  Block argmin = wavefront shuffle
// reduction on (distance, index) pairs + one LDS hop across the 4 waves.
// ---------------------------------------------------------------------------------------------------------------
constexpr int VQ_ROWS = 8;

__global__ __launch_bounds__(256) void vq_argmin_kernel(const float *__restrict__ x, int ldx, int M,
                                                        const float *__restrict__ cb, const float *__restrict__ csq,
                                                        int ncode, int dim, int64_t *idx, long idx_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *xs = sm;                              // [VQ_ROWS][dim]
    float *xsq = sm + VQ_ROWS * dim;             // [VQ_ROWS]
    float *rd = xsq + VQ_ROWS;                   // [4][VQ_ROWS]
    int *ri = reinterpret_cast<int *>(rd + 4 * VQ_ROWS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * VQ_ROWS;
    for (int i = tid; i < VQ_ROWS * dim; i += 256) {
        int r = i / dim, c = i - r * dim;
        xs[i] = (m0 + r < M) ? x[(long)(m0 + r) * ldx + c] : 0.f;
    }
    __syncthreads();
    if (tid < VQ_ROWS) {
        float s = 0.f;
        for (int c = 0; c < dim; ++c) s += xs[tid * dim + c] * xs[tid * dim + c];
        xsq[tid] = s;
    }
    __syncthreads();

    float best[VQ_ROWS];
    int bidx[VQ_ROWS];
#pragma unroll
    for (int r = 0; r < VQ_ROWS; ++r) { best[r] = INFINITY; bidx[r] = 0x7fffffff; }

    for (int j = tid; j < ncode; j += 256) {
        float dot[VQ_ROWS];
#pragma unroll
        for (int r = 0; r < VQ_ROWS; ++r) dot[r] = 0.f;
        const float4 *e = reinterpret_cast<const float4 *>(cb + (long)j * dim);
        for (int c4 = 0; c4 < dim / 4; ++c4) {
            const float4 ev = e[c4];
#pragma unroll
            for (int r = 0; r < VQ_ROWS; ++r) {
                const float4 xv = *reinterpret_cast<const float4 *>(&xs[r * dim + c4 * 4]);
                dot[r] = fmaf(xv.x, ev.x, dot[r]);
                dot[r] = fmaf(xv.y, ev.y, dot[r]);
                dot[r] = fmaf(xv.z, ev.z, dot[r]);
                dot[r] = fmaf(xv.w, ev.w, dot[r]);
            }
        }
        const float ee = csq[j];
#pragma unroll
        for (int r = 0; r < VQ_ROWS; ++r) {
            const float d = (xsq[r] + ee) - 2.0f * dot[r];
            if (d < best[r]) { best[r] = d; bidx[r] = j; }
        }
    }
#pragma unroll
    for (int r = 0; r < VQ_ROWS; ++r) {
        float d = best[r];
        int j = bidx[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(d, off);
            const int oj = __shfl_xor(j, off);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        if (lane == 0) { rd[wave * VQ_ROWS + r] = d; ri[wave * VQ_ROWS + r] = j; }
    }
    __syncthreads();
    if (tid < VQ_ROWS && m0 + tid < M) {
        float d = rd[tid];
        int j = ri[tid];
        for (int w = 1; w < 4; ++w) {
            const float od = rd[w * VQ_ROWS + tid];
            const int oj = ri[w * VQ_ROWS + tid];
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        idx[(long)(m0 + tid) * idx_stride] = j;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// vq_argmin, LDS-staged form (dim = 64: the VQ-VAE's embedding width).  The kernel above lets every thread pull its own code
// rows from L2 — a wave load touches 64 rows x 16 B, and a workgroup of 8 query rows reads the whole 512 KB codebook.  Here:
//   * a workgroup serves 4 x RW query rows and walks the codebook in TILES of 64 codes, staged through LDS by coalesced 16-byte
//     loads (a tile is 16 KB contiguous) into rows pitched 68 floats — lane l then reads code l of the tile with ds_read_b128,
//     conflict-free — and double-buffered: tile t + 1 is on its way while tile t is multiplied;
//   * lane = code, wave = RW query rows: the query values are WAVE-UNIFORM, so they come through the scalar unit (s_load) and
//     enter the FMAs as scalar operands — no LDS traffic, no broadcast, 64 v_fmac per (row, tile) against the lane's 64 code
//     registers;
//   * a lane keeps its running (distance, index) per row over the tiles it sees (codes l, l + 64, ...: ascending, strict '<'
//     keeps the lowest index), one wavefront reduction per row at the end (ties -> lowest index).
// Same arithmetic as above, operation for operation — dot as the c-ascending fmaf chain, (|x|^2 + |e|^2) - 2 dot, |x|^2 summed
// in c order — so the two kernels return the same index for every row (tests/test_gpu_parity.py::test_vq_argmin_lds_form).
// ---------------------------------------------------------------------------------------------------------------
constexpr int VQ_TILE = 64, VQ_DIM = 64, VQ_PITCH = VQ_DIM + 4;

template <int RW>
__global__ __launch_bounds__(256) void vq_argmin_lds_kernel(const float *__restrict__ x, int ldx, int M, const float *__restrict__ cb,
                                                            const float *__restrict__ csq, int ncode, int64_t *__restrict__ idx, long idx_stride) {
    __shared__ __attribute__((aligned(16))) float tile[2][VQ_TILE][VQ_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m0 = blockIdx.x * (4 * RW) + wave * RW;   // this wave's first query row (wave-uniform)
    const int ntile = (ncode + VQ_TILE - 1) / VQ_TILE;

    // |x|^2 of the wave's rows, in the order the kernel above sums it (wave-uniform values: every lane computes the same number)
    float xsq[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        const float *xr = x + (long)(m0 + r < M ? m0 + r : 0) * ldx;
        float sq = 0.f;
        for (int c = 0; c < VQ_DIM; ++c) sq += xr[c] * xr[c];
        xsq[r] = sq;
    }
    float best[RW];
    int bidx[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) { best[r] = INFINITY; bidx[r] = 0x7fffffff; }

    // staging: a tile is 64 x 64 floats = 1024 16-byte chunks, 4 per thread; chunk q -> row q / 16, columns 4 (q % 16) ..
    f32x4 st[4];
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, row = q >> 4;
            st[i] = t * VQ_TILE + row < ncode ? *reinterpret_cast<const f32x4 *>(cb + ((long)t * VQ_TILE + row) * VQ_DIM + (q & 15) * 4)
                                              : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            *reinterpret_cast<f32x4 *>(&tile[buf][q >> 4][(q & 15) * 4]) = st[i];
        }
    };
    fetch(0);
    park(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntile) fetch(t + 1);   // in flight under this tile's FMAs
        f32x4 e[VQ_DIM / 4];
#pragma unroll
        for (int c4 = 0; c4 < VQ_DIM / 4; ++c4) e[c4] = *reinterpret_cast<const f32x4 *>(&tile[buf][lane][c4 * 4]);
        const int j = t * VQ_TILE + lane;
        const float ee = j < ncode ? csq[j] : 0.f;
#pragma unroll
        for (int r = 0; r < RW; ++r) {
            const float *xr = x + (long)(m0 + r < M ? m0 + r : 0) * ldx;   // wave-uniform address: scalar loads
            float dot = 0.f;
#pragma unroll
            for (int c4 = 0; c4 < VQ_DIM / 4; ++c4) {
                dot = fmaf(xr[c4 * 4 + 0], e[c4][0], dot);
                dot = fmaf(xr[c4 * 4 + 1], e[c4][1], dot);
                dot = fmaf(xr[c4 * 4 + 2], e[c4][2], dot);
                dot = fmaf(xr[c4 * 4 + 3], e[c4][3], dot);
            }
            const float d = (xsq[r] + ee) - 2.0f * dot;
            if (j < ncode && d < best[r]) { best[r] = d; bidx[r] = j; }
        }
        if (t + 1 < ntile) park(buf ^ 1);   // the other buffer was last read two iterations ago, behind the barrier below
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        float d = best[r];
        int j = bidx[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(d, off);
            const int oj = __shfl_xor(j, off);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        if (lane == 0 && m0 + r < M) idx[(long)(m0 + r) * idx_stride] = j;
    }
}

hipError_t launch_vq_argmin(const float *x, int ldx, int M, const float *codebook, const float *code_sq, int ncode,
                            int dim, int64_t *idx, long idx_stride, hipStream_t stream) {
    if (dim % 4 != 0) return hipErrorInvalidValue;
    if (dim == VQ_DIM && knobs().vq_lds && (reinterpret_cast<uintptr_t>(codebook) & 15) == 0) {
        // 32 rows per workgroup once that still fills the chip, else 8 (the batch-of-32 call: 2 400 rows)
        if (M >= 32 * 512) hipLaunchKernelGGL(vq_argmin_lds_kernel<8>, dim3((M + 31) / 32), dim3(256), 0, stream, x, ldx, M, codebook, code_sq, ncode, idx, idx_stride);
        else hipLaunchKernelGGL(vq_argmin_lds_kernel<2>, dim3((M + 7) / 8), dim3(256), 0, stream, x, ldx, M, codebook, code_sq, ncode, idx, idx_stride);
        return hipGetLastError();
    }
    size_t smem = (VQ_ROWS * dim + VQ_ROWS + 4 * VQ_ROWS) * sizeof(float) + 4 * VQ_ROWS * sizeof(int);
    hipLaunchKernelGGL(vq_argmin_kernel, dim3((M + VQ_ROWS - 1) / VQ_ROWS), dim3(256), smem, stream, x, ldx, M,
                       codebook, code_sq, ncode, dim, idx, idx_stride);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// vq_argmin for a MIXED pass, both networks in one launch (talkshow_hip.h, "given poses").  vq_argmin_lds_kernel with
//   * blockIdx.y = network (net0 + blockIdx.y: a one-network launch names its network through net0): {z, codebook, |e|^2, output column};
//   * a validity bit per row: row m = b * H + h is valid iff h < lens[b] >> 2.  b, h and lens[b] are functions of blockIdx and the wave
//     index only, so the bits sit in scalar registers like the query rows themselves and every test on them is wave-uniform;
//   * output straight into the interleaved code block codes (B, Hout, 2): the arg-min of a valid row, -1 for an invalid one.
// A workgroup without a valid row stores its -1s and returns before it touches the codebook.  In a partly valid workgroup every wave walks
// every tile and reaches every barrier; an invalid row skips its |x|^2, its FMAs and its reduction — its row of z is never addressed, so no
// clamped address exists that could point outside z.  Arithmetic: that of vq_argmin_lds_kernel, statement for statement.
// ---------------------------------------------------------------------------------------------------------------
template <int RW>
__global__ __launch_bounds__(256) void vq_argmin_pair_lds_kernel(const VqPairParams p, int net0) {
    static_assert(4 * RW <= 32, "the workgroup's validity bits live in one 32-bit word");
    __shared__ __attribute__((aligned(16))) float tile[2][VQ_TILE][VQ_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = net0 + blockIdx.y;
    const float *__restrict__ x = p.z[n], *__restrict__ cb = p.cb[n], *__restrict__ csq = p.csq[n];
    const int ncode = p.ncode[n], M = p.B * p.H;
    const int g0 = blockIdx.x * (4 * RW);               // the workgroup's first row
    int64_t *__restrict__ out = p.codes + n;
    auto slot = [&](int m) -> int64_t * {
        const int b = m / p.H, h = m - b * p.H;
        return out + ((long)b * p.Hout + h) * 2;
    };

    // validity of the workgroup's 4 RW rows (every wave computes all of them: the early return below is workgroup-uniform without a barrier)
    unsigned wg = 0;
    {
        int b = g0 / p.H, h = g0 - b * p.H;
        int hb = g0 < M ? (p.lens[b] >> 2) : 0;
        for (int i = 0; i < 4 * RW && g0 + i < M; ++i) {
            if (h < hb) wg |= 1u << i;
            if (++h == p.H) {
                h = 0;
                ++b;
                if (g0 + i + 1 < M) hb = p.lens[b] >> 2;
            }
        }
    }
    wg = __builtin_amdgcn_readfirstlane(wg);
    if (wg == 0) {
        if (tid < 4 * RW && g0 + tid < M) *slot(g0 + tid) = -1;
        return;
    }
    const int m0 = g0 + wave * RW;                       // this wave's first query row (wave-uniform)
    const unsigned vm = (wg >> (wave * RW)) & ((1u << RW) - 1u);
    const int ntile = (ncode + VQ_TILE - 1) / VQ_TILE;

    float xsq[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        xsq[r] = 0.f;
        if ((vm >> r) & 1u) {
            const float *xr = x + (long)(m0 + r) * VQ_DIM;
            float sq = 0.f;
            for (int c = 0; c < VQ_DIM; ++c) sq += xr[c] * xr[c];
            xsq[r] = sq;
        }
    }
    float best[RW];
    int bidx[RW];
#pragma unroll
    for (int r = 0; r < RW; ++r) { best[r] = INFINITY; bidx[r] = 0x7fffffff; }

    f32x4 st[4];
    auto fetch = [&](int t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i, row = q >> 4;
            st[i] = t * VQ_TILE + row < ncode ? *reinterpret_cast<const f32x4 *>(cb + ((long)t * VQ_TILE + row) * VQ_DIM + (q & 15) * 4)
                                              : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = tid + 256 * i;
            *reinterpret_cast<f32x4 *>(&tile[buf][q >> 4][(q & 15) * 4]) = st[i];
        }
    };
    fetch(0);
    park(0);
    __syncthreads();
    for (int t = 0; t < ntile; ++t) {
        const int buf = t & 1;
        if (t + 1 < ntile) fetch(t + 1);
        const int j = t * VQ_TILE + lane;
        if (vm) {                                        // a wave without a valid row only stages tiles and keeps the barriers
            f32x4 e[VQ_DIM / 4];
#pragma unroll
            for (int c4 = 0; c4 < VQ_DIM / 4; ++c4) e[c4] = *reinterpret_cast<const f32x4 *>(&tile[buf][lane][c4 * 4]);
            const float ee = j < ncode ? csq[j] : 0.f;
#pragma unroll
            for (int r = 0; r < RW; ++r) {
                if (!((vm >> r) & 1u)) continue;         // wave-uniform: skip the FMAs, never a barrier
                const float *xr = x + (long)(m0 + r) * VQ_DIM;   // wave-uniform address: scalar loads
                float dot = 0.f;
#pragma unroll
                for (int c4 = 0; c4 < VQ_DIM / 4; ++c4) {
                    dot = fmaf(xr[c4 * 4 + 0], e[c4][0], dot);
                    dot = fmaf(xr[c4 * 4 + 1], e[c4][1], dot);
                    dot = fmaf(xr[c4 * 4 + 2], e[c4][2], dot);
                    dot = fmaf(xr[c4 * 4 + 3], e[c4][3], dot);
                }
                const float d = (xsq[r] + ee) - 2.0f * dot;
                if (j < ncode && d < best[r]) { best[r] = d; bidx[r] = j; }
            }
        }
        if (t + 1 < ntile) park(buf ^ 1);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < RW; ++r) {
        if (m0 + r >= M) continue;
        if (!((vm >> r) & 1u)) {
            if (lane == 0) *slot(m0 + r) = -1;
            continue;
        }
        float d = best[r];
        int j = bidx[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(d, off);
            const int oj = __shfl_xor(j, off);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        if (lane == 0) *slot(m0 + r) = j;
    }
}

// vq_argmin_kernel (any dim % 4 == 0, any ncode) for one network of a mixed pass: the fallback of the kernel above.  Invalid rows are staged
// as zeros without being read and stored as -1; a workgroup without a valid row returns before its first barrier.
__global__ __launch_bounds__(256) void vq_argmin_masked_kernel(const float *__restrict__ x, int B, int H, int Hout, const int *__restrict__ lens,
                                                               const float *__restrict__ cb, const float *__restrict__ csq, int ncode, int dim,
                                                               int64_t *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float *xs = sm;                              // [VQ_ROWS][dim]
    float *xsq = sm + VQ_ROWS * dim;             // [VQ_ROWS]
    float *rd = xsq + VQ_ROWS;                   // [4][VQ_ROWS]
    int *ri = reinterpret_cast<int *>(rd + 4 * VQ_ROWS);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int M = B * H, m0 = blockIdx.x * VQ_ROWS;
    unsigned vm = 0;
    for (int r = 0; r < VQ_ROWS && m0 + r < M; ++r) {
        const int b = (m0 + r) / H, h = (m0 + r) - b * H;
        if (h < (lens[b] >> 2)) vm |= 1u << r;
    }
    auto slot = [&](int m) -> int64_t * {
        const int b = m / H, h = m - b * H;
        return out + ((long)b * Hout + h) * 2;
    };
    if (vm == 0) {
        if (tid < VQ_ROWS && m0 + tid < M) *slot(m0 + tid) = -1;
        return;
    }
    for (int i = tid; i < VQ_ROWS * dim; i += 256) {
        int r = i / dim, c = i - r * dim;
        xs[i] = ((vm >> r) & 1u) ? x[(long)(m0 + r) * dim + c] : 0.f;
    }
    __syncthreads();
    if (tid < VQ_ROWS) {
        float s = 0.f;
        for (int c = 0; c < dim; ++c) s += xs[tid * dim + c] * xs[tid * dim + c];
        xsq[tid] = s;
    }
    __syncthreads();

    float best[VQ_ROWS];
    int bidx[VQ_ROWS];
#pragma unroll
    for (int r = 0; r < VQ_ROWS; ++r) { best[r] = INFINITY; bidx[r] = 0x7fffffff; }

    for (int j = tid; j < ncode; j += 256) {
        float dot[VQ_ROWS];
#pragma unroll
        for (int r = 0; r < VQ_ROWS; ++r) dot[r] = 0.f;
        const float4 *e = reinterpret_cast<const float4 *>(cb + (long)j * dim);
        for (int c4 = 0; c4 < dim / 4; ++c4) {
            const float4 ev = e[c4];
#pragma unroll
            for (int r = 0; r < VQ_ROWS; ++r) {
                const float4 xv = *reinterpret_cast<const float4 *>(&xs[r * dim + c4 * 4]);
                dot[r] = fmaf(xv.x, ev.x, dot[r]);
                dot[r] = fmaf(xv.y, ev.y, dot[r]);
                dot[r] = fmaf(xv.z, ev.z, dot[r]);
                dot[r] = fmaf(xv.w, ev.w, dot[r]);
            }
        }
        const float ee = csq[j];
#pragma unroll
        for (int r = 0; r < VQ_ROWS; ++r) {
            const float d = (xsq[r] + ee) - 2.0f * dot[r];
            if (d < best[r]) { best[r] = d; bidx[r] = j; }
        }
    }
#pragma unroll
    for (int r = 0; r < VQ_ROWS; ++r) {
        float d = best[r];
        int j = bidx[r];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float od = __shfl_xor(d, off);
            const int oj = __shfl_xor(j, off);
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        if (lane == 0) { rd[wave * VQ_ROWS + r] = d; ri[wave * VQ_ROWS + r] = j; }
    }
    __syncthreads();
    if (tid < VQ_ROWS && m0 + tid < M) {
        float d = rd[tid];
        int j = ri[tid];
        for (int w = 1; w < 4; ++w) {
            const float od = rd[w * VQ_ROWS + tid];
            const int oj = ri[w * VQ_ROWS + tid];
            if (od < d || (od == d && oj < j)) { d = od; j = oj; }
        }
        *slot(m0 + tid) = ((vm >> tid) & 1u) ? (int64_t)j : (int64_t)-1;
    }
}

hipError_t launch_vq_argmin_pair_masked(const VqPairParams &p, int form, hipStream_t stream) {
    if (!p.lens || !p.codes || p.B < 1 || p.H < 1 || p.Hout < p.H || (long)p.B * p.H > 0x7fffffffl) return hipErrorInvalidValue;
    for (int n = 0; n < 2; ++n)
        if (!p.z[n] || !p.cb[n] || !p.csq[n] || p.ncode[n] < 1 || p.dim[n] < 4 || p.dim[n] % 4) return hipErrorInvalidValue;
    const int M = p.B * p.H;
    const bool lds = p.dim[0] == VQ_DIM && p.dim[1] == VQ_DIM && p.ncode[0] == p.ncode[1] && knobs().vq_lds &&
                     ((reinterpret_cast<uintptr_t>(p.cb[0]) | reinterpret_cast<uintptr_t>(p.cb[1])) & 15) == 0;
    if (form == 0) form = knobs().vq_pair ? 1 : 2;
    if (!lds || form == 3) {
        for (int n = 0; n < 2; ++n) {
            const int dim = p.dim[n];
            size_t smem = (VQ_ROWS * dim + VQ_ROWS + 4 * VQ_ROWS) * sizeof(float) + 4 * VQ_ROWS * sizeof(int);
            hipLaunchKernelGGL(vq_argmin_masked_kernel, dim3((M + VQ_ROWS - 1) / VQ_ROWS), dim3(256), smem, stream, p.z[n], p.B, p.H, p.Hout,
                               p.lens, p.cb[n], p.csq[n], p.ncode[n], dim, p.codes + n);
            hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    }
    // the row-count switch of launch_vq_argmin; one launch over both networks, or one per network
    const int nl = form == 2 ? 2 : 1, ny = form == 2 ? 1 : 2;
    for (int l = 0; l < nl; ++l) {
        if (M >= 32 * 512) hipLaunchKernelGGL(vq_argmin_pair_lds_kernel<8>, dim3((M + 31) / 32, ny), dim3(256), 0, stream, p, l);
        else hipLaunchKernelGGL(vq_argmin_pair_lds_kernel<2>, dim3((M + 7) / 8, ny), dim3(256), 0, stream, p, l);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

__global__ void row_sqnorm_kernel(const float *e, int n, int dim, float *out) {
    int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    float s = 0.f;
    for (int c = 0; c < dim; ++c) s += e[(long)j * dim + c] * e[(long)j * dim + c];
    out[j] = s;
}
hipError_t launch_row_sqnorm(const float *e, int n, int dim, float *out, hipStream_t stream) {
    hipLaunchKernelGGL(row_sqnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, e, n, dim, out);
    return hipGetLastError();
}

// one wave per row, 16-byte lanes
__global__ __launch_bounds__(256) void gather_rows_kernel(const float *__restrict__ table, int ld_table,
                                                          const int64_t *__restrict__ idx, long idx_stride, int M,
                                                          int width, float *__restrict__ out, int ldo, int nrows) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int64_t r = idx[(long)m * idx_stride];
    float4 *dst = reinterpret_cast<float4 *>(out + (long)m * ldo);
    if (r < 0 || r >= nrows) {   // nn.Embedding would raise IndexError; here: memory-safe and loud (a row of NaNs)
        const float q = __builtin_nanf("");
        for (int c = lane; c < width / 4; c += 64) dst[c] = make_float4(q, q, q, q);
        return;
    }
    const float4 *src = reinterpret_cast<const float4 *>(table + r * ld_table);
    for (int c = lane; c < width / 4; c += 64) dst[c] = src[c];
}
hipError_t launch_gather_rows(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M,
                              int width, float *out, int ldo, hipStream_t stream) {
    if (width % 4 || ld_table % 4 || ldo % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((M + 3) / 4), dim3(256), 0, stream, table, ld_table, idx, idx_stride,
                       M, width, out, ldo, nrows);
    return hipGetLastError();
}

// speaker style (talkshow_hip.h): the class-conditioning rows of a window of code rows from float WEIGHTS in place of integer labels.
// One wave per (row of the window, clip slot, layer): out[l][rr][slot][0..W) = sum over c ascending of w[slot][r][c] * E_l[c][0..W), every
// product and every sum rounded to fp32 on its own (__fmul_rn / __fadd_rn: no FMA contraction), a weight of exactly 0 skipped — its table
// row is not loaded — and +0.0 where every weight is 0.  The weight row's address depends on blockIdx only, so its loads are scalar and
// the zero-skip is a uniform branch.  S == 1: one weight row per slot serves every row.  With a length table, a row at or beyond the
// slot's own H_b = lens[slot] >> len_shr takes the weights of row H_b - 1 (rows carried to a chunk's end read finite data).
__global__ __launch_bounds__(64) void style_rows_kernel(const StyleRowsParams p) {
    const int rr = blockIdx.x / p.slots, slot = blockIdx.x - rr * p.slots, l = blockIdx.y;
    int r = p.r0 + rr;
    if (p.lens) r = min(r, (p.lens[slot] >> p.len_shr) - 1);
    r = max(min(r, p.S - 1), 0);
    const float *__restrict__ wrow = p.weights + ((long)slot * p.S + r) * p.w_ld;
    const float *__restrict__ tab = p.tables + (long)l * p.NC * p.W;
    float4 *__restrict__ dst = reinterpret_cast<float4 *>(p.out + (long)l * p.out_l_stride + (long)rr * p.out_r_stride + (long)slot * p.W);
    for (int q = threadIdx.x; q < p.W / 4; q += 64) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        bool any = false;
        for (int c = 0; c < p.NC; ++c) {
            const float wc = wrow[c];
            if (wc == 0.f) continue;
            const float4 e = reinterpret_cast<const float4 *>(tab + (long)c * p.W)[q];
            const float4 t = make_float4(__fmul_rn(wc, e.x), __fmul_rn(wc, e.y), __fmul_rn(wc, e.z), __fmul_rn(wc, e.w));
            acc = any ? make_float4(__fadd_rn(acc.x, t.x), __fadd_rn(acc.y, t.y), __fadd_rn(acc.z, t.z), __fadd_rn(acc.w, t.w)) : t;
            any = true;
        }
        dst[q] = acc;
    }
}
hipError_t launch_style_rows(const StyleRowsParams &p, hipStream_t stream) {
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!p.tables || !p.weights || !p.out || p.NL < 1 || p.NC < 1 || p.W < 4 || p.W % 4 || p.S < 1 || p.n < 1 || p.slots < 1 || p.r0 < 0 ||
        p.w_ld < p.NC || p.out_l_stride % 4 || p.out_r_stride % 4 || !al16(p.tables) || !al16(p.out) || (p.S > 1 && p.r0 + p.n > p.S) ||
        (long)p.n * p.slots > 0x7fffffffl || p.NL > 65535 || (p.lens && p.len_shr < 0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(style_rows_kernel, dim3((unsigned)(p.n * p.slots), (unsigned)p.NL), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// gather_rows_kernel for a padded batch of clips of different lengths (mixed passes): rows beyond a clip's own length become zero rows —
// what the conv gather substitutes past the end of a clip run alone — and their index is never read
__global__ __launch_bounds__(256) void gather_rows_masked_kernel(const float *__restrict__ table, int ld_table,
                                                                 const int64_t *__restrict__ idx, long idx_stride, int M, int width,
                                                                 float *__restrict__ out, int ldo, int nrows, int L,
                                                                 const int *__restrict__ lens, int len_shr) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = m / L, t = m - b * L;
    float4 *dst = reinterpret_cast<float4 *>(out + (long)m * ldo);
    if (t >= (lens[b] >> len_shr)) {
        for (int c = lane; c < width / 4; c += 64) dst[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int64_t r = idx[(long)m * idx_stride];
    if (r < 0 || r >= nrows) {   // a bad index INSIDE the clip stays loud
        const float q = __builtin_nanf("");
        for (int c = lane; c < width / 4; c += 64) dst[c] = make_float4(q, q, q, q);
        return;
    }
    const float4 *src = reinterpret_cast<const float4 *>(table + r * ld_table);
    for (int c = lane; c < width / 4; c += 64) dst[c] = src[c];
}
hipError_t launch_gather_rows_masked(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M,
                                     int width, float *out, int ldo, int L, const int *lens, int len_shr, hipStream_t stream) {
    if (width % 4 || ld_table % 4 || ldo % 4 || L < 1 || M % L || !lens || len_shr < 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_masked_kernel, dim3((M + 3) / 4), dim3(256), 0, stream, table, ld_table, idx, idx_stride, M, width,
                       out, ldo, nrows, L, lens, len_shr);
    return hipGetLastError();
}

__global__ void pad_rows_masked_kernel(const float *__restrict__ src, int lds_, int c, float *__restrict__ dst, int ldd, int cpad,
                                       long M, int L, const int *__restrict__ lens) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cpad) return;
    const long m = i / cpad;
    const int k = (int)(i - m * cpad);
    const int b = (int)(m / L), t = (int)(m - (long)b * L);
    dst[m * ldd + k] = (k < c && t < lens[b]) ? src[m * lds_ + k] : 0.f;   // the padding is not read: NaNs there never enter a product
}
hipError_t launch_pad_rows_masked(const float *src, int lds_, int c, float *dst, int ldd, int cpad, int B, int L, const int *lens,
                                  hipStream_t stream) {
    const long M = (long)B * L, n = M * cpad;
    if (!lens || L < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pad_rows_masked_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, lds_, c, dst, ldd, cpad, M, L, lens);
    return hipGetLastError();
}

__global__ void mask_codes_kernel(int64_t *codes, int B, int H, const int *__restrict__ lens) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, r = i - b * H;
    if (r >= (lens[b] >> 2)) codes[2l * i] = codes[2l * i + 1] = -1;
}
hipError_t launch_mask_codes(int64_t *codes, int B, int H, const int *lens, hipStream_t stream) {
    hipLaunchKernelGGL(mask_codes_kernel, dim3((unsigned)((B * H + 255) / 256)), dim3(256), 0, stream, codes, B, H, lens);
    return hipGetLastError();
}

__global__ void iota_i64_kernel(int64_t *dst, int n, int64_t first) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = first + i;
}
hipError_t launch_iota_i64(int64_t *dst, int n, int64_t first, hipStream_t stream) {
    hipLaunchKernelGGL(iota_i64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, dst, n, first);
    return hipGetLastError();
}

__global__ void pad_rows_kernel(const float *__restrict__ src, int lds_, int c, float *__restrict__ dst, int ldd,
                                int cpad, long M) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * cpad) return;
    const long m = i / cpad;
    const int k = (int)(i - m * cpad);
    dst[m * ldd + k] = k < c ? src[m * lds_ + k] : 0.f;
}
hipError_t launch_pad_rows(const float *src, int lds_, int c, float *dst, int ldd, int cpad, long M, hipStream_t stream) {
    const long n = M * cpad;
    hipLaunchKernelGGL(pad_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, lds_, c, dst,
                       ldd, cpad, M);
    return hipGetLastError();
}

// Whole-body output assembly (scripts/demo.py:207-229 + data_utils/lower_body.py:68-87): per frame
//   p232 = [jaw = face[0:3] | body/hand 129 (last frame repeated / trimmed to the face length) | expression = face[3:103]]
//   out265 = [p[0:3] lp[0:15] p[3:6] lp[15:21] p[6:9] lp[21:27] p[9:12] lp[27:33] p[12:232]]
// One thread per output element; pure copies, HBM-bound (1.9 KB per frame).
struct AssembleParams {
    const float *body;   // (B, Tb, 129)
    const float *face;   // (B, Tf, 103)
    float *out;          // (B, Tf, 265)
    int B, Tb, Tf;
    float lp[33];        // the fixed lower-body pose block
};
__global__ void assemble_full_kernel(const AssembleParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)p.B * p.Tf * 265;
    if (i >= n) return;
    const int c = (int)(i % 265);
    const long bt = i / 265;
    const int t = (int)(bt % p.Tf), b = (int)(bt / p.Tf);
    // column of the 232-vector this output column copies, or -(k+1) for lower-pose constant k
    int src;
    if (c < 3) src = c;
    else if (c < 18) src = -(c - 3 + 1);
    else if (c < 21) src = c - 15;
    else if (c < 27) src = -(15 + c - 21 + 1);
    else if (c < 30) src = c - 21;
    else if (c < 36) src = -(21 + c - 30 + 1);
    else if (c < 39) src = c - 27;
    else if (c < 45) src = -(27 + c - 39 + 1);
    else src = c - 33;
    float v;
    if (src < 0) {
        v = p.lp[-src - 1];
    } else if (src < 3) {
        v = p.face[((long)b * p.Tf + t) * 103 + src];
    } else if (src < 132) {
        const int tb = t < p.Tb ? t : p.Tb - 1;
        v = p.body[((long)b * p.Tb + tb) * 129 + (src - 3)];
    } else {
        v = p.face[((long)b * p.Tf + t) * 103 + 3 + (src - 132)];
    }
    p.out[i] = v;
}
hipError_t launch_assemble_full(const float *body, const float *face, const float *lower_pose33, int B, int Tb, int Tf,
                                float *out, hipStream_t stream) {
    AssembleParams p;
    p.body = body; p.face = face; p.out = out; p.B = B; p.Tb = Tb; p.Tf = Tf;
    for (int k = 0; k < 33; ++k) p.lp[k] = lower_pose33[k];
    const long n = (long)B * Tf * 265;
    hipLaunchKernelGGL(assemble_full_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// The same assembly for a padded batch (mixed passes): clip b has tb[b] body frames of Tb and tf[b] face frames of Tf.  Row t < tf[b] is the
// row of assemble_full_kernel on the clip alone (body frame min(t, tb[b] - 1)); rows at or beyond tf[b] are written as 0.  A kernel of its
// own: the one above keeps its code.
struct AssembleMixedParams {
    const float *body;   // (B, Tb, 129)
    const float *face;   // (B, Tf, 103)
    const int *tb, *tf;  // (B,) device tables
    float *out;          // (B, Tf, 265)
    int B, Tb, Tf;
    float lp[33];
};
__global__ void assemble_full_len_kernel(const AssembleMixedParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long n = (long)p.B * p.Tf * 265;
    if (i >= n) return;
    const int c = (int)(i % 265);
    const long bt = i / 265;
    const int t = (int)(bt % p.Tf), b = (int)(bt / p.Tf);
    if (t >= p.tf[b]) {
        p.out[i] = 0.f;
        return;
    }
    int src;
    if (c < 3) src = c;
    else if (c < 18) src = -(c - 3 + 1);
    else if (c < 21) src = c - 15;
    else if (c < 27) src = -(15 + c - 21 + 1);
    else if (c < 30) src = c - 21;
    else if (c < 36) src = -(21 + c - 30 + 1);
    else if (c < 39) src = c - 27;
    else if (c < 45) src = -(27 + c - 39 + 1);
    else src = c - 33;
    float v;
    if (src < 0) {
        v = p.lp[-src - 1];
    } else if (src < 3) {
        v = p.face[((long)b * p.Tf + t) * 103 + src];
    } else if (src < 132) {
        int last = p.tb[b] - 1;                       // (clamped into the buffer: the tables exist on the device only)
        last = last < 0 ? 0 : (last >= p.Tb ? p.Tb - 1 : last);
        const int tb = t < last ? t : last;
        v = p.body[((long)b * p.Tb + tb) * 129 + (src - 3)];
    } else {
        v = p.face[((long)b * p.Tf + t) * 103 + 3 + (src - 132)];
    }
    p.out[i] = v;
}
hipError_t launch_assemble_full_lens(const float *body, const int *tb, const float *face, const int *tf, const float *lower_pose33, int B,
                                     int Tb, int Tf, float *out, hipStream_t stream) {
    AssembleMixedParams p;
    p.body = body; p.face = face; p.tb = tb; p.tf = tf; p.out = out; p.B = B; p.Tb = Tb; p.Tf = Tf;
    for (int k = 0; k < 33; ++k) p.lp[k] = lower_pose33[k];
    const long n = (long)B * Tf * 265;
    hipLaunchKernelGGL(assemble_full_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

__global__ void i64_to_i32_kernel(const int64_t *src, int *dst, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (int)src[i];
}
hipError_t launch_i64_to_i32(const int64_t *src, int *dst, long n, hipStream_t stream) {
    hipLaunchKernelGGL(i64_to_i32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, src, dst, n);
    return hipGetLastError();
}

// three 64-bit words (the sampler's {seed, first clip index, Philox position base}) written by a kernel whose ARGUMENTS carry
// them: arguments are copied when the launch is queued, so — unlike an asynchronous copy out of host memory — nothing on the
// host has to outlive the call, however many calls are queued behind each other on the stream
__global__ void set_words3_kernel(uint64_t *dst, uint64_t a, uint64_t b, uint64_t c) {
    dst[0] = a;
    dst[1] = b;
    dst[2] = c;
}
hipError_t launch_set_words3(uint64_t *dst, uint64_t a, uint64_t b, uint64_t c, hipStream_t stream) {
    hipLaunchKernelGGL(set_words3_kernel, dim3(1), dim3(1), 0, stream, dst, a, b, c);
    return hipGetLastError();
}

// "slot restart" (kernels.h: SlotResetParams).  One workgroup per (listed slot, layer l) and one more per slot (blockIdx.y == NL) for what
// has no layer: the token ring, the layer-0 look-ahead sums and the origin.  Every row is written as float4 (4D and 2D are multiples of 4:
// D % 32 == 0).  A slot or label outside its range writes nothing (the host has refused such a call already).
__global__ __launch_bounds__(256) void slot_reset_kernel(const SlotResetParams p) {
    const int slot = p.slots[blockIdx.x], l = (int)blockIdx.y, tid = threadIdx.x;
    if (slot < 0 || slot >= p.B) return;
    const int D4 = 4 * p.D, D2 = 2 * p.D, r = p.row;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l == p.NL) {
        if (tid < 6) {   // rows r-1, r-2, r-3 of the ring, both columns
            const int rr = r - 1 - (tid >> 1);
            if (rr >= 0) p.tok32[((long)slot * p.R + rr % p.R) * 2 + (tid & 1)] = -1;
        }
        if (tid == 6) p.row_origin[slot] = r;
        float4 *q1 = reinterpret_cast<float4 *>(p.Q1 + ((long)(r & 3) * p.B + slot) * D4);
        float4 *q0a = reinterpret_cast<float4 *>(p.Q0 + ((long)(r & 3) * p.B + slot) * D4);
        float4 *q0b = reinterpret_cast<float4 *>(p.Q0 + ((long)((r + 1) & 3) * p.B + slot) * D4);
        for (int q = tid; q < D4 / 4; q += 256) q1[q] = q0a[q] = q0b[q] = zero;
        return;
    }
    if (l >= 1) {
        const float4 *bv = reinterpret_cast<const float4 *>(p.bv + (long)l * D4);
        float4 *dst = reinterpret_cast<float4 *>(p.P + ((long)(l * 2 + (r & 1)) * p.B + slot) * D4);
        for (int q = tid; q < D4 / 4; q += 256) dst[q] = bv[q];
    }
    if (p.labels) {
        const int label = p.labels[blockIdx.x];
        if (label < 0 || label >= p.NC) return;
        const float4 *src = reinterpret_cast<const float4 *>(p.tables + ((long)l * p.NC + label) * D2);
        float4 *dst = reinterpret_cast<float4 *>(p.CR + ((long)l * p.B + slot) * D2);
        for (int q = tid; q < D2 / 4; q += 256) dst[q] = src[q];
    }
}
hipError_t launch_slot_reset(const SlotResetParams &p, hipStream_t stream) {
    auto al16 = [](const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    if (!p.slots || !p.tok32 || !p.Q1 || !p.Q0 || !p.P || !p.CR || !p.bv || !p.tables || !p.row_origin || p.n < 1 || p.B < 1 || p.n > p.B ||
        p.row < 0 || p.D < 4 || p.D % 4 || p.NL < 1 || p.NL > 65534 || p.NC < 1 || p.R < 4 || !al16(p.Q1) || !al16(p.Q0) || !al16(p.P) ||
        !al16(p.CR) || !al16(p.bv) || !al16(p.tables))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_reset_kernel, dim3((unsigned)p.n, (unsigned)(p.NL + 1)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// "slot state" (kernels.h: SlotSaveParams, SlotLoadParams), in slot_reset_kernel's shape: one workgroup per (listed slot, layer l) for
// P(l) and CR[l], and one more per slot (blockIdx.y == NL) for the token ring, the Q rows and the histories; float4 rows, plain vector
// loads and stores.  Every index is bounded by the launcher's checks and the slot / state-index tests below.
__global__ __launch_bounds__(256) void slot_save_kernel(const SlotSaveParams p) {
    const int slot = p.slots[blockIdx.x], l = (int)blockIdx.y, tid = threadIdx.x;
    if (slot < 0 || slot >= p.B) return;
    const int D4 = 4 * p.D, D2 = 2 * p.D, r = p.row;
    const SlotStateLayout L = slot_state_layout(p.D, p.NL);
    float *out = p.state + (long)blockIdx.x * L.words;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    if (l == p.NL) {
        int32_t *tok = reinterpret_cast<int32_t *>(out + L.tok), *rep = reinterpret_cast<int32_t *>(out + L.rep);
        if (tid < SLOT_STATE_TOK_WORDS) {   // rows r-1, r-2, r-3 of the ring, both columns; a row below 0 is the restart's -1
            int v = 0;
            if (tid < 6) {
                const int rr = r - 1 - (tid >> 1);
                v = rr >= 0 ? p.tok32[((long)slot * p.R + rr % p.R) * 2 + (tid & 1)] : -1;
            }
            tok[tid] = v;
        }
        if (tid >= 128) {   // both histories by age: entry k is the code of row r-1-k
            const int k = tid - 128, col = k >> 6, age = k & 63;
            rep[k] = age < p.hist[blockIdx.x] ? p.rep_ring[((long)slot * 2 + col) * SAMPLE_REP_RING + ((r - 1 - age) & (SAMPLE_REP_RING - 1))] : -1;
        }
        const float4 *q1 = reinterpret_cast<const float4 *>(p.Q1 + ((long)(r & 3) * p.B + slot) * D4);
        const float4 *q0a = reinterpret_cast<const float4 *>(p.Q0 + ((long)(r & 3) * p.B + slot) * D4);
        const float4 *q0b = reinterpret_cast<const float4 *>(p.Q0 + ((long)((r + 1) & 3) * p.B + slot) * D4);
        float4 *o1 = reinterpret_cast<float4 *>(out + L.q1), *oa = reinterpret_cast<float4 *>(out + L.q0a), *ob = reinterpret_cast<float4 *>(out + L.q0b);
        for (int q = tid; q < D4 / 4; q += 256) {   // what rows r and r + 1 of the session do not read may never have been written
            float4 a = q1[q], b = q0a[q], c = q0b[q];
            if (r < 2) a = zero, c = zero;
            if (r < 3) b = zero;
            o1[q] = a, oa[q] = b, ob[q] = c;
        }
        return;
    }
    if (l >= 1) {
        const float4 *src = reinterpret_cast<const float4 *>(r == 0 ? p.bv + (long)l * D4 : p.P + ((long)(l * 2 + (r & 1)) * p.B + slot) * D4);
        float4 *dst = reinterpret_cast<float4 *>(out + L.p + (long)(l - 1) * D4);
        for (int q = tid; q < D4 / 4; q += 256) dst[q] = src[q];
    }
    const float *cr = p.CR + ((long)l * p.B + slot) * D2;
    if (p.open_labels) {   // a session at row 0: the first step has not written CR yet; its rows will be the open label's
        const int64_t label = p.open_labels[slot];
        if (label < 0 || label >= p.NC) return;
        cr = p.tables + ((long)l * p.NC + label) * D2;
    }
    const float4 *src = reinterpret_cast<const float4 *>(cr);
    float4 *dst = reinterpret_cast<float4 *>(out + L.cr + (long)l * D2);
    for (int q = tid; q < D2 / 4; q += 256) dst[q] = src[q];
}
__global__ __launch_bounds__(256) void slot_load_kernel(const SlotLoadParams p) {
    const int slot = p.slots[blockIdx.x], idx = p.index[blockIdx.x], l = (int)blockIdx.y, tid = threadIdx.x;
    if (slot < 0 || slot >= p.B || idx < 0 || idx >= p.n_states) return;
    const int D4 = 4 * p.D, D2 = 2 * p.D, r = p.row;
    const SlotStateLayout L = slot_state_layout(p.D, p.NL);
    const float *in = p.state + (long)idx * L.words;
    if (l == p.NL) {
        const int32_t *tok = reinterpret_cast<const int32_t *>(in + L.tok), *rep = reinterpret_cast<const int32_t *>(in + L.rep);
        if (tid < 6) {
            const int rr = r - 1 - (tid >> 1);
            if (rr >= 0) p.tok32[((long)slot * p.R + rr % p.R) * 2 + (tid & 1)] = tok[tid];
        }
        if (tid == 6) p.row_origin[slot] = p.origin[blockIdx.x];
        if (tid >= 128) {
            const int k = tid - 128, col = k >> 6, age = k & 63;
            p.rep_ring[((long)slot * 2 + col) * SAMPLE_REP_RING + ((r - 1 - age) & (SAMPLE_REP_RING - 1))] = rep[k];
        }
        float4 *q1 = reinterpret_cast<float4 *>(p.Q1 + ((long)(r & 3) * p.B + slot) * D4);
        float4 *q0a = reinterpret_cast<float4 *>(p.Q0 + ((long)(r & 3) * p.B + slot) * D4);
        float4 *q0b = reinterpret_cast<float4 *>(p.Q0 + ((long)((r + 1) & 3) * p.B + slot) * D4);
        const float4 *i1 = reinterpret_cast<const float4 *>(in + L.q1), *ia = reinterpret_cast<const float4 *>(in + L.q0a),
                     *ib = reinterpret_cast<const float4 *>(in + L.q0b);
        for (int q = tid; q < D4 / 4; q += 256) q1[q] = i1[q], q0a[q] = ia[q], q0b[q] = ib[q];
        return;
    }
    if (l >= 1) {
        const float4 *src = reinterpret_cast<const float4 *>(in + L.p + (long)(l - 1) * D4);
        float4 *dst = reinterpret_cast<float4 *>(p.P + ((long)(l * 2 + (r & 1)) * p.B + slot) * D4);
        for (int q = tid; q < D4 / 4; q += 256) dst[q] = src[q];
    }
    const float4 *src = reinterpret_cast<const float4 *>(in + L.cr + (long)l * D2);
    float4 *dst = reinterpret_cast<float4 *>(p.CR + ((long)l * p.B + slot) * D2);
    for (int q = tid; q < D2 / 4; q += 256) dst[q] = src[q];
}
static bool slot_al16(const void *q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }
hipError_t launch_slot_save(const SlotSaveParams &p, hipStream_t stream) {
    if (!p.slots || !p.hist || !p.tok32 || !p.Q1 || !p.Q0 || !p.P || !p.CR || !p.bv || !p.rep_ring || !p.state || p.n < 1 || p.B < 1 || p.n > p.B ||
        p.row < 0 || p.D < 4 || p.D % 4 || p.NL < 1 || p.NL > 65534 || p.R < 4 || (p.open_labels && (!p.tables || p.NC < 1)) || !slot_al16(p.Q1) ||
        !slot_al16(p.Q0) || !slot_al16(p.P) || !slot_al16(p.CR) || !slot_al16(p.bv) || !slot_al16(p.state) || (p.open_labels && !slot_al16(p.tables)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_save_kernel, dim3((unsigned)p.n, (unsigned)(p.NL + 1)), dim3(256), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_slot_load(const SlotLoadParams &p, hipStream_t stream) {
    if (!p.slots || !p.index || !p.origin || !p.tok32 || !p.Q1 || !p.Q0 || !p.P || !p.CR || !p.rep_ring || !p.row_origin || !p.state || p.n < 1 ||
        p.B < 1 || p.n > p.B || p.n_states < 1 || p.row < 0 || p.D < 4 || p.D % 4 || p.NL < 1 || p.NL > 65534 || p.R < 4 || !slot_al16(p.Q1) ||
        !slot_al16(p.Q0) || !slot_al16(p.P) || !slot_al16(p.CR) || !slot_al16(p.state))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_load_kernel, dim3((unsigned)p.n, (unsigned)(p.NL + 1)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

// test aid: out[i] = gate_act(v[i], p[i]) — the chain kernels' gate on given operands (tests measure it against tanh * sigmoid in float64)
__global__ void gate_act_kernel(const float *v, const float *p, float *out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gate_act(v[i], p[i]);
}
hipError_t launch_gate_act(const float *v, const float *p, float *out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(gate_act_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v, p, out, n);
    return hipGetLastError();
}
// test aid: out[i] = gelu_fast(v[i]) — the face generator's GELU epilogue on given operands (tests measure it against float64 erf)
__global__ void gelu_kernel(const float *v, float *out, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = gelu_fast(v[i]);
}
hipError_t launch_gelu(const float *v, float *out, long n, hipStream_t stream) {
    hipLaunchKernelGGL(gelu_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, v, out, n);
    return hipGetLastError();
}

// measurement aid: one wave that sleeps and, every `window_ticks` of the 100 MHz wall clock, records (wall ticks, shader cycles)
// since the previous record — the shader clock the chip actually runs at while other streams load it
__global__ void clock_sample_kernel(unsigned long long *out, int n, unsigned long long window_ticks) {
    if (threadIdx.x != 0) return;
    unsigned long long w0 = wall_clock64(), c0 = clock64();
    const unsigned long long wstart = w0;
    for (int i = 0; i < n; ++i) {
        unsigned long long w1;
        do {
            __builtin_amdgcn_s_sleep(64);
            w1 = wall_clock64();
        } while (w1 - w0 < window_ticks);
        const unsigned long long c1 = clock64();
        out[3 * i] = w1 - wstart;
        out[3 * i + 1] = w1 - w0;
        out[3 * i + 2] = c1 - c0;
        w0 = w1;
        c0 = c1;
    }
}
hipError_t launch_clock_sample(unsigned long long *out, int n, unsigned long long window_ticks, hipStream_t stream) {
    hipLaunchKernelGGL(clock_sample_kernel, dim3(1), dim3(64), 0, stream, out, n, window_ticks);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// samplers: one workgroup per clip over V logits.  Twelve __global__ entries, two bodies: sample_plain_body<LP, GIVEN> behind
// sample_kernel, sample_lp_kernel, sample_given_kernel and sample_lp_given_kernel; sample_ctl_body<FAST, LP, GIVEN> behind the four
// sample_ctl_kernel and the four sample_ctl_given_kernel instantiations.  An entry declares its LDS and calls its body; the variants
// differ by `if constexpr` inside a body, so the rule below is stated on the device once per body and its blocks once.
//   greedy   : argmax, ties -> lowest index (torch.argmax on CPU returns the first maximum).
//   sampling : inverse CDF of softmax(logits).  p_v ∝ exp(l_v - max); thread t owns the contiguous chunk
//              [t*V/256, (t+1)*V/256), sums it left to right; thread 0 prefix-sums the 256 chunk sums left to right;
//              the draw is the first index whose running sum exceeds u * total.  oracle/talkshow_oracle.py
//              (`sample_inverse_cdf`) restates exactly this summation structure AND the exponential (`det_expf` below: fp32
//              multiplies / adds only), so the draw of a given uniform is the same index bit for bit.
// ---------------------------------------------------------------------------------------------------------------
__device__ inline void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                     uint32_t &o0) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o0 = c0;
}

// ---- the blocks both sampler bodies (sample_plain_body, sample_ctl_body) are made of, each written once ----

__device__ __forceinline__ const float *sample_row(const SampleParams &p, int b) {
    return p.logits + (long)b * (p.logit_stride ? p.logit_stride : (long)p.V);
}
// the row load of the vector path: a thread's 8 consecutive logits from two 16-byte loads, up front — the samplers sit on the dependent
// chain, and a load-per-iteration loop costs one memory round trip per element
__device__ __forceinline__ void sample_load8(const float *lg, int v0, float (&x)[8]) {
    const f32x4 lo = *reinterpret_cast<const f32x4 *>(lg + v0), hi = *reinterpret_cast<const f32x4 *>(lg + v0 + 4);
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = lo[k]; x[4 + k] = hi[k]; }
}
// logits_copy: every thread stores its chunk [v0, v1) (vector path: the 8 registers)
__device__ __forceinline__ void sample_copy_row(const SampleParams &p, int b, bool fast, const float *lg, const float (&x)[8], int v0, int v1) {
    if (!p.logits_copy) return;
    float *dst = p.logits_copy + (long)b * p.copy_stride;
    if (fast) {
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[v0 + k] = x[k];
    } else {
        for (int v = v0; v < v1; ++v) dst[v] = lg[v];
    }
}
// workgroup arg-max over every thread's own (best, bi); ties -> lowest index.  Uses sf[0..3] / si[0..3] between two barriers of its own.
__device__ __forceinline__ void sample_argmax(float &best, int &bi, float *sf, int *si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bi, off);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    if (lane == 0) { sf[wave] = best; si[wave] = bi; }
    __syncthreads();
    best = sf[0]; bi = si[0];
    for (int w = 1; w < 4; ++w)
        if (sf[w] > best || (sf[w] == best && si[w] < bi)) { best = sf[w]; bi = si[w]; }
    __syncthreads();
}
// the source of u for clip b in a drawing mode: the injected uniform, or Philox at (position, clip)
__device__ __forceinline__ float sample_uniform(const SampleParams &p, int b) {
    if (p.mode == TS_SAMPLE_UNIFORMS) return p.uniforms[(long)b * p.u_stride];
    const uint64_t seed = p.dyn ? p.dyn[0] : p.seed;
    // a mixed pass orders its clips by length: the subsequence then comes from a per-clip table, so that a clip's draws keep
    // depending on its GLOBAL index only
    const uint64_t clip = p.clip_table ? (uint64_t)p.clip_table[b] : (uint64_t)((p.dyn ? (int64_t)p.dyn[1] : p.clip_index0) + b);
    // "slot restart": the counter word is the position inside the slot's current clip (null: the session's own, as ever)
    const uint32_t pos = p.position + (p.dyn ? (uint32_t)p.dyn[2] : 0u) - (p.row_origin ? 2u * (uint32_t)p.row_origin[b] : 0u);
    uint32_t r;
    philox4x32_10(pos, (uint32_t)clip, (uint32_t)(clip >> 32), 0u, (uint32_t)seed, (uint32_t)(seed >> 32), r);
    return (float)(r >> 8) * (1.0f / 16777216.0f);
}
// thread 0, after every thread t stored its chunk sum in sf[t + 1]: the 256 sums left to right, sf[t] = sum of the chunks < t; returns the
// total (= sf[256]).  LAST: hi[t] holds chunk t's highest kept index or -1, and last receives the highest kept index of the row.
template <bool LAST = false>
__device__ __forceinline__ float sample_prefix_sum(float *sf, const int *hi = nullptr, int *last = nullptr) {
    float c = 0.f;
    int l = 0;
    sf[0] = 0.f;
    for (int t = 1; t <= 256; ++t) {
        c += sf[t]; sf[t] = c;
        if constexpr (LAST) {
            if (hi[t - 1] >= 0) l = hi[t - 1];
        }
    }
    if constexpr (LAST) *last = l;
    return c;
}
// a thread's chunk sum of p_v ∝ exp(l_v - max), left to right
__device__ __forceinline__ float sample_chunk_sum(bool fast, const float *lg, const float (&x)[8], int v0, int v1, float best) {
    float s = 0.f;
    if (fast) {
#pragma unroll
        for (int k = 0; k < 8; ++k) s += det_expf(x[k] - best);
    } else {
        for (int v = v0; v < v1; ++v) s += det_expf(lg[v] - best);
    }
    return s;
}
// the draw, after sample_prefix_sum: the owner — the first chunk whose inclusive prefix exceeds thr (the last non-empty chunk if none
// does) — repeats its running sum and finds the first index that crosses thr.  One barrier; the index travels through si[0].
__device__ __forceinline__ int sample_crossing(bool fast, const float *lg, const float (&x)[8], int v0, int v1, int V, float best, float thr,
                                               const float *sf, int *si) {
    const int tid = threadIdx.x;
    const bool mine = (sf[tid] <= thr) && (thr < sf[tid + 1] || tid == 255);
    if (mine && v0 < V) {
        float c = sf[tid];
        int k = v1 - 1;
        if (fast) {
            bool found = false;
#pragma unroll
            for (int j = 0; j < 8; ++j) {   // same running sum as the loop below; the first crossing is latched
                c += det_expf(x[j] - best);
                if (!found && c > thr) { k = v0 + j; found = true; }
            }
        } else {
            for (int v = v0; v < v1; ++v) {
                c += det_expf(lg[v] - best);
                if (c > thr) { k = v; break; }
            }
        }
        si[0] = k;
    } else if (mine) {
        si[0] = V - 1;
    }
    __syncthreads();
    return si[0];
}
// given rows (talkshow_hip.h): clip b of a pass brings G_b = rows[b] code rows that are TAKEN, not drawn.  A workgroup is FORCED iff its
// absolute position 2 row + column — the Philox counter word, the dynamic base word of a replayed graph included — is below 2 G_b and
// ("kept positions") the pass brings no mask or the mask's byte of this (clip, row, column) is not 0: a workgroup-uniform decision from
// kernel arguments, two uniform loads and, with a mask, one byte every lane loads from the same address (made scalar by readfirstlane, so
// the branches on it stay scalar branches), taken before any barrier.  The byte is read below 2 G_b only; keep == nullptr executes the
// loads and compares there were before the mask existed.  A given code is compared, never used as an address; outside [0, V) it leaves
// -1 in tok32 (the chain's gathers read a row of zeros for a negative index).
__device__ __forceinline__ bool given_forced(const SampleParams &p, const int *rows, const unsigned char *keep, long keep_stride, int b) {
    const uint32_t pos = p.position + (p.dyn ? (uint32_t)p.dyn[2] : 0u);
    const int G = rows[b];
    if (!(G > 0 && (uint64_t)pos < 2ull * (uint64_t)G)) return false;
    if (!keep) return true;
    return __builtin_amdgcn_readfirstlane((int)keep[(long)b * keep_stride]) != 0;
}
__device__ __forceinline__ int given_token(long long code, int V) { return code >= 0 && code < (long long)V ? (int)code : -1; }
// the log-probability (talkshow_hip.h, "log-probabilities") of the row's code, stored by the ONE thread that owns the code's index: d = the
// fp32 argument of the code's exponential, S = the row's total.  A code outside [0, V) finds no owner: thread 0 then stores NaN.
// kept = false: a given code the filters removed has weight 0 in the distribution the row would have been drawn from, log(0).
__device__ __forceinline__ void sample_store_logprob(float *out, float d, float S, bool kept = true) {
    *out = kept ? (float)((double)d - log((double)S)) : (float)log(0.0);
}
__device__ __forceinline__ void sample_store_unowned(float *out, long long code, int V) {
    if (code < 0 || code >= (long long)V) *out = __uint_as_float(0x7fc00000u);
}

// ---------------------------------------------------------------------------------------------------------------
// The body of the four samplers without controls.  Flags:
//   LP     also the log-probability of the code: greedy and teacher forced compute the total S too (the sampler's summation structure).
//          The logit of the code c is picked up by the thread that OWNS index c (a 64-bit comparison against its chunk): c is never an
//          address.  One fp64 log on one lane, one 4-byte store.  Without LP a teacher-forced workgroup copies its code and leaves.
//   GIVEN  a forced workgroup takes its code from `given`, writes it to tok32 and codes, reads no uniform and draws nothing: without LP
//          it leaves right after the copy, with LP it scores the code the way LP scores a teacher-forced one.  An unforced workgroup
//          executes the arithmetic of the kernel without GIVEN, operation for operation.
// Each kernel keeps the predicate of its vector path: chunk == 8 and V a multiple of 8 without LP, V == 2048 on a 16-byte aligned row
// with it.  The body is inlined into its four __global__ entries; what was compared against the six separate kernels it replaces is
// recorded in DESIGN.md §5 ("One body per sampler family").
// ---------------------------------------------------------------------------------------------------------------
template <bool LP, bool GIVEN>
__device__ __forceinline__ void sample_plain_body(const SampleParams &p, float *logprob, long lp_stride, const int *rows, const int64_t *given,
                                                  long given_stride, const unsigned char *keep, long keep_stride, float *sf, int *si,
                                                  float &s_thr) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const float *lg = sample_row(p, b);
    bool forced = false;   // workgroup-uniform, ahead of every barrier
    if constexpr (GIVEN && LP) forced = given_forced(p, rows, keep, keep_stride, b);

    // Every thread owns `chunk` consecutive logits [v0, v1); for the production vocabulary (V = 2048: chunk = 8) they stay in registers
    const int chunk = (p.V + 255) / 256;
    const int v0 = tid * chunk, v1 = min(v0 + chunk, p.V);
    bool fast;
    if constexpr (LP) fast = p.V == 2048 && (reinterpret_cast<uintptr_t>(lg) & 15) == 0;
    else fast = chunk == 8 && (p.V & 7) == 0;
    float x[8];
    if (fast) sample_load8(lg, v0, x);
    sample_copy_row(p, b, fast, lg, x, v0, v1);

    if constexpr (!LP && GIVEN) {
        if (given_forced(p, rows, keep, keep_stride, b)) {
            if (tid == 0) {
                const long long code = given[(long)b * given_stride];
                p.tok32[(long)b * p.tok_stride] = given_token(code, p.V);
                p.codes[(long)b * p.code_stride] = code;
            }
            return;
        }
    } else if constexpr (!LP) {
        if (p.mode == TS_TEACHER_FORCED) {
            if (tid == 0) p.tok32[(long)b * p.tok_stride] = (int)p.codes[(long)b * p.code_stride];
            return;
        }
    }

    // ---- max / argmax (needed by every mode); ties -> lowest index ----
    float best = -INFINITY;
    int bi = 0x7fffffff;
    if (fast) {
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (x[k] > best) { best = x[k]; bi = v0 + k; }
    } else {
        for (int v = v0; v < v1; ++v) {
            const float t = lg[v];
            if (t > best) { best = t; bi = v; }
        }
    }
    sample_argmax(best, bi, sf, si);

    if constexpr (!LP) {
        int choice = bi;
        if (p.mode != TS_SAMPLE_GREEDY) {
            const float u = sample_uniform(p, b);
            sf[tid + 1] = sample_chunk_sum(fast, lg, x, v0, v1, best);
            __syncthreads();
            if (tid == 0) s_thr = u * sample_prefix_sum(sf);
            __syncthreads();
            choice = sample_crossing(fast, lg, x, v0, v1, p.V, best, s_thr, sf, si);
        }
        if (tid == 0) {
            p.tok32[(long)b * p.tok_stride] = choice;
            p.codes[(long)b * p.code_stride] = choice;
        }
    } else {
        // ---- the total, in every mode: sf[t] = sum of the chunks < t, sf[256] = S ----
        sf[tid + 1] = sample_chunk_sum(fast, lg, x, v0, v1, best);
        __syncthreads();
        const bool draws = !forced && (p.mode == TS_SAMPLE_UNIFORMS || p.mode == TS_SAMPLE_PHILOX);
        if (tid == 0) {
            const float u = draws ? sample_uniform(p, b) : 0.f;   // the uniform of a forced row is never read
            s_thr = u * sample_prefix_sum(sf);
        }
        __syncthreads();

        const bool taken = GIVEN ? forced : p.mode == TS_TEACHER_FORCED;   // the code is read, not chosen
        long long code;   // 64 bits: a teacher-forced or given code is compared, never truncated
        if (taken) code = GIVEN ? given[(long)b * given_stride] : p.codes[(long)b * p.code_stride];
        else if (!draws) code = bi;
        else code = sample_crossing(fast, lg, x, v0, v1, p.V, best, s_thr, sf, si);

        float *out = logprob + (long)b * lp_stride;
        if (code >= (long long)v0 && code < (long long)v1) {   // the owner of index `code`: exactly one thread, or none when it is out of range
            float lc = 0.f;
            if (fast) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    if ((long long)(v0 + k) == code) lc = x[k];
            } else {
                for (int v = v0; v < v1; ++v)
                    if ((long long)v == code) lc = lg[v];
            }
            sample_store_logprob(out, lc - best, sf[256]);
        }
        if (tid == 0) {
            sample_store_unowned(out, code, p.V);
            p.tok32[(long)b * p.tok_stride] = GIVEN ? given_token(code, p.V) : (int)code;
            if (GIVEN || p.mode != TS_TEACHER_FORCED) p.codes[(long)b * p.code_stride] = code;
        }
    }
}

__global__ __launch_bounds__(256) void sample_kernel(const SampleParams p) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    sample_plain_body<false, false>(p, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr);
}
__global__ __launch_bounds__(256) void sample_lp_kernel(const SampleLpParams lp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    sample_plain_body<true, false>(lp.s, lp.logprob, lp.lp_stride, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr);
}
__global__ __launch_bounds__(256) void sample_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    sample_plain_body<false, true>(gp.c.s, nullptr, 0, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si, s_thr);
}
__global__ __launch_bounds__(256) void sample_lp_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    sample_plain_body<true, true>(gp.c.s, gp.c.logprob, gp.c.lp_stride, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si,
                                  s_thr);
}

hipError_t launch_sample(const SampleParams &p, hipStream_t stream) {
    hipLaunchKernelGGL(sample_kernel, dim3(p.B), dim3(256), 0, stream, p);
    return hipGetLastError();
}
hipError_t launch_sample_lp(const SampleLpParams &p, hipStream_t stream) {
    if (!p.logprob || p.s.V < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_lp_kernel, dim3(p.s.B), dim3(256), 0, stream, p);
    return hipGetLastError();
}

__global__ void mask_logprob_kernel(float *lp, int B, int H, const int *__restrict__ lens) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * H) return;
    const int b = i / H, r = i - b * H;
    if (r >= (lens[b] >> 2)) lp[2l * i] = lp[2l * i + 1] = 0.f;
}
hipError_t launch_mask_logprob(float *logprob, int B, int H, const int *lens, hipStream_t stream) {
    hipLaunchKernelGGL(mask_logprob_kernel, dim3((unsigned)((B * H + 255) / 256)), dim3(256), 0, stream, logprob, B, H, lens);
    return hipGetLastError();
}

// stage 1: lane t of clip b adds rows t, t + 256, ... (ascending) of the clip's own rows, each column by itself
__global__ __launch_bounds__(LOGPROB_SUM_LANES) void logprob_sums_partial(const float *__restrict__ lp, int H, const int *__restrict__ lens,
                                                                          double *__restrict__ part) {
    const int b = blockIdx.x, t = threadIdx.x;
    const int Hb = lens ? min(H, max(lens[b] >> 2, 0)) : H;
    const float *row = lp + (size_t)b * H * 2;
    double s0 = 0.0, s1 = 0.0;
    for (int r = t; r < Hb; r += LOGPROB_SUM_LANES) {
        s0 += (double)row[2 * r];
        s1 += (double)row[2 * r + 1];
    }
    part[((size_t)b * LOGPROB_SUM_LANES + t) * 2] = s0;
    part[((size_t)b * LOGPROB_SUM_LANES + t) * 2 + 1] = s1;
}
// stage 2: the 256 partials of a clip in ascending order; out[b] = {body, hand, body + hand}
__global__ void logprob_sums_final(const double *__restrict__ part, int B, double *__restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double s0 = 0.0, s1 = 0.0;
    for (int t = 0; t < LOGPROB_SUM_LANES; ++t) {
        s0 += part[((size_t)b * LOGPROB_SUM_LANES + t) * 2];
        s1 += part[((size_t)b * LOGPROB_SUM_LANES + t) * 2 + 1];
    }
    out[3 * b] = s0;
    out[3 * b + 1] = s1;
    out[3 * b + 2] = s0 + s1;
}
hipError_t launch_logprob_sums(const float *logprob, int B, int H, const int *lens, double *scratch, double *out, hipStream_t stream) {
    if (!logprob || !scratch || !out || B < 1 || H < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(logprob_sums_partial, dim3(B), dim3(LOGPROB_SUM_LANES), 0, stream, logprob, H, lens, scratch);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(logprob_sums_final, dim3((B + 63) / 64), dim3(64), 0, stream, scratch, B, out);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------
// sampler with per-clip controls (temperature, top-k, top-p): the rule is stated in talkshow_hip.h (ts_sampling, steps 1-5) and restated
// in talkshow_amd/sampling.py.  A body of its own (sample_ctl_body below) behind kernels of their own: a pass without controls keeps the
// launches of the plain body's kernels.  The two bodies share the blocks above (row load, arg-max, the source of u, the prefix sum, the
// given-row decision, the log-probability store) and nothing else.
//
// Same launch shape (one workgroup of 256 threads per clip, thread t owns the contiguous chunk [t*ceil(V/256), ...)); at V = 2048 the 8
// logits of a thread, their order keys and their quantised weights stay in registers.  The kept set is a PREFIX of the ranking (logit
// descending, ties by index ascending), so it is found by radix select instead of a sort:
//   key(l)   the logit's bits mapped to an unsigned integer of the same order (-0 counts as +0);
//   q(w)     floor(w * 2^31), the weight as an integer: integer sums do not depend on the order they are taken in, so the LDS atomics
//            below are deterministic (no floating-point atomics anywhere);
//   a level  256-bin histogram of the next 8 key bits over the tokens that match the bits chosen so far; a bin holds count and mass in
//            ONE 64-bit word (count << 44 | mass: V * 2^31 < 2^44 for every V <= SAMPLE_CTL_MAX_V = 8191, which the launcher enforces), i.e. one LDS atomic per token and level.  After the barrier every
//            WAVE scans all 256 bins by itself (lane l: bins 4l .. 4l+3, one wave suffix scan) — the chosen bin is then workgroup-uniform
//            without a second barrier or an LDS round trip.
// top-k descends by count to the key K* of rank k-1, top-p by mass to the lowest key whose mass-above is below the threshold; four levels
// each, level 0 shared.  Ties at the two boundary keys are resolved in index order with one packed prefix count over the threads.
// A neutral record (1, 1, 0) skips all of it (workgroup-uniform) and computes the plain body's bits.
// ---------------------------------------------------------------------------------------------------------------
typedef unsigned long long ctl_u64;
constexpr int CTL_CNT_SHIFT = 44;   // a bin = count << 44 | mass; mass = sums of floor(w * 2^31)
static_assert(((ctl_u64)SAMPLE_CTL_MAX_V << 31) < (1ull << CTL_CNT_SHIFT), "the mass of a full row must stay below the count field");
static_assert(SAMPLE_CTL_MAX_V < 65536, "the packed tie counters hold 16 bits each");
constexpr ctl_u64 CTL_MASS_MASK = (1ull << CTL_CNT_SHIFT) - 1;

__device__ inline uint32_t ctl_key(float l) {
    uint32_t b = __float_as_uint(l);
    if (b == 0x80000000u) b = 0u;   // -0 ranks with +0
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float ctl_unkey(uint32_t k) { return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k); }
// step 1: subtract, multiply (two fp32 operations: a difference times a factor cannot contract), det_expf
__device__ inline float ctl_arg(float l, float m, float inv_t) {
#pragma clang fp contract(off)
    const float d = l - m;
    return d * inv_t;
}
__device__ inline float ctl_weight(float l, float m, float inv_t) { return det_expf(ctl_arg(l, m, inv_t)); }
__device__ inline uint32_t ctl_quant(float w) { return (uint32_t)(w * 2147483648.0f); }   // w in [0, 1]: the product is exact, the cast truncates

// packed sum of all 256 bins (every lane gets it)
__device__ inline ctl_u64 ctl_hist_total(const ctl_u64 *h, int lane) {
    ctl_u64 s = h[4 * lane] + h[4 * lane + 1] + h[4 * lane + 2] + h[4 * lane + 3];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
// One level of a descent, computed by every wave for itself.  acc = packed (count, mass) of the tokens ABOVE the bins of this level.
//   by count: the bin b with  count above b < target <= count above b + count(b)
//   by mass : the lowest non-empty bin b with  mass above b < target
// Returns b (-1 if none: malformed rows only) and adds the bins above b to acc.
__device__ inline int ctl_pick_bin(const ctl_u64 *h, int lane, bool by_mass, ctl_u64 target, ctl_u64 &acc) {
    ctl_u64 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = h[4 * lane + j];
    const ctl_u64 own = v[0] + v[1] + v[2] + v[3];
    ctl_u64 suf = own;   // inclusive suffix sum over the lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const ctl_u64 o = __shfl_down(suf, off);
        if (lane + off < 64) suf += o;
    }
    ctl_u64 above = suf - own + acc;
    int pick = -1;
    ctl_u64 pick_above = 0;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        const ctl_u64 cnt = v[j] >> CTL_CNT_SHIFT;
        const bool ok = by_mass ? (cnt > 0 && (above & CTL_MASS_MASK) < target)
                                : ((above >> CTL_CNT_SHIFT) < target && target <= (above >> CTL_CNT_SHIFT) + cnt);
        if (ok) { pick = 4 * lane + j; pick_above = above; }   // walking down: the lowest qualifying bin of the lane stays
        above += v[j];
    }
    const ctl_u64 vote = __ballot(pick >= 0);
    const int src = vote ? __ffsll(vote) - 1 : 0;             // lowest lane = lowest bin
    acc = __shfl(pick_above, src);
    return __shfl(pick, src);
}

// what a token needs to decide whether the filters keep it (workgroup-uniform except the two tie counters' start values)
struct CtlSel {
    bool need_k, need_p, p_top;   // p_top: no token ranks above key Kp (its first tie is rank 0, always kept)
    uint32_t Kk, Kp;              // boundary keys of top-k / top-p
    int ntie_k;                   // ties at Kk that top-k keeps (lowest indices first)
    ctl_u64 mgt_p, q_p, Tq;       // mass above Kp, quantised weight of a token at Kp, threshold ceil(p * mass kept by top-k)
};
// tokens are visited in index order; jk / jp count the ties met so far at the two boundary keys (start: the ties owned by lower threads)
__device__ inline bool ctl_keep(const CtlSel &S, uint32_t ky, int &jk, int &jp) {
    bool ok = true;
    if (S.need_k) {
        if (ky < S.Kk) ok = false;
        else if (ky == S.Kk) ok = jk++ < S.ntie_k;
    }
    if (S.need_p) {
        if (ky < S.Kp) ok = false;
        else if (ky == S.Kp) {
            const int j = jp++;
            ok = ok && ((S.p_top && j == 0) || S.mgt_p + (ctl_u64)j * S.q_p < S.Tq);
        }
    }
    return ok;
}

// step 0b of the "repetition penalty" (talkshow_hip.h) for one token: c = how often the window met it
__device__ __forceinline__ float rep_penalise(float l, int c, float presence, float frequency) {
#pragma clang fp contract(off)
    if (c <= 0) return l;                      // a token the window has not met keeps its bits
    const float f = frequency * (float)c;      // three fp32 operations, each rounded on its own
    const float g = presence + f;
    return l - g;
}

// the rule of "guidance" (talkshow_hip.h) for one token: difference, product and sum, each rounded on its own
__device__ __forceinline__ float guide_mix(float l, float lq, float scale) {
#pragma clang fp contract(off)
    const float d = l - lq;
    const float t = scale * d;
    return l + t;
}
// the value sample_store_logprob stores, for a workgroup that stores it twice (GUIDE)
__device__ __forceinline__ float sample_logprob_value(float d, float S, bool kept = true) {
    return kept ? (float)((double)d - log((double)S)) : (float)log(0.0);
}

// ---- "alternatives" (talkshow_hip.h): what the ALT flag of the body below adds ----
// a token's place in step 2's ranking as one integer: a higher key first, a lower index first among equal keys.  Never 0 for a token
__device__ __forceinline__ ctl_u64 alt_pack(uint32_t key, int v) { return ((ctl_u64)key << 32) | (ctl_u64)(0xffffffffu - (uint32_t)v); }
__device__ __forceinline__ int alt_index(ctl_u64 pk) { return (int)(0xffffffffu - (uint32_t)pk); }
// E += w * d: one fp32 product, one fp32 addition
__device__ __forceinline__ float alt_acc(float e, float w, float d) {
#pragma clang fp contract(off)
    const float t = w * d;
    return e + t;
}
struct AltLds {
    ctl_u64 top[2][4];             // a round's wave maxima, double buffered: one barrier per round
    ctl_u64 ck;                    // the packed place of the row's code (0: a code outside [0, V))
    float d[SAMPLE_ALT_MAX];       // d_j of the alternatives, stored by their owners
    int code[SAMPLE_ALT_MAX];      // their indices, -1 beyond the allowed tokens
    float sa[256], se[256];        // chunk sums of w and of w * d over all tokens
    float tot[2];                  // S_all, E
    int rank;
};

// ALT: the rank of the row's code and the four stores; two barriers, reached by a forced workgroup and an unforced one alike.  logit: the
// body's own accessor of l''
template <class L>
__device__ __forceinline__ void alt_finish(const SampleAltParams *ap, AltLds *al, long long code, int b, int v0, int v1, int n, const L &logit) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (code >= (long long)v0 && code < (long long)v1) {   // the owner of the code's index (a code outside [0, V) has none)
#pragma unroll 8
        for (int k = 0; k < n; ++k)
            if ((long long)(v0 + k) == code) al->ck = alt_pack(ctl_key(logit(k)), v0 + k);
    }
    __syncthreads();
    const ctl_u64 ck = al->ck;
    if (ck) {   // workgroup-uniform
        int cnt = 0;
#pragma unroll 8
        for (int k = 0; k < n; ++k) cnt += alt_pack(ctl_key(logit(k)), v0 + k) > ck ? 1 : 0;   // all V tokens, banned ones included
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
        if (lane == 0) atomicAdd(&al->rank, cnt);
    }
    __syncthreads();
    const long e = (long)b * ap->stride;
    const float S_all = al->tot[0];
    if (tid < ap->n) {
        const int c = al->code[tid];
        ap->codes[e * ap->n + tid] = c;
        ap->logprob[e * ap->n + tid] = c >= 0 ? (float)((double)al->d[tid] - log((double)S_all)) : (float)log(0.0);
    }
    if (tid == 64) ap->entropy[e] = (float)(log((double)S_all) - (double)al->tot[1] / (double)S_all);
    if (tid == 65) ap->rank[e] = ck ? al->rank : -1;
}
// the chunk's sums of w and of w * d over all tokens: no member, no register without ALT
template <bool ON> struct AltSums { float s = 0.f, e = 0.f; };
template <> struct AltSums<false> {};

// The body of the eight samplers with controls.  Flags:
//   FAST   V = 2048 on 16-byte aligned rows (the launchers decide): every thread owns 8 logits, held in registers from two 16-byte loads
//   LP     also write the log-probability of the row's code under the distribution it was drawn from (cp.logprob; talkshow_hip.h,
//          "log-probabilities"): d_c - log S with d_c the argument of the code's exponential and S the total of the kept weights, both
//          already here
//   GIVEN  given rows: without LP a forced workgroup copies its code and leaves ahead of everything; with it, it runs steps 1-4 and the
//          sums of step 5 as an unforced one does (the thread that owns the given code notes whether the filters kept it), then writes
//          d_c - log S for a kept code and log(0) for a code the filters removed.  An unforced workgroup executes the arithmetic of the
//          kernel without GIVEN, operation for operation.
//   BIAS   "code bias" (talkshow_hip.h, step 0): a clip slot whose bias_index is not negative adds its table's row of this column to the
//          logits, one fp32 addition per token, and runs every step on the sums l'; a token with l' = -inf is never kept.  The row copy
//          stays the network's l.  The index is workgroup-uniform: a slot with -1 reads no table and executes the arithmetic of the
//          kernel without BIAS, operation for operation.  BIAS = false compiles to what the body was before the flag existed.
//   REP    "repetition penalty" (talkshow_hip.h, step 0b): a clip slot whose record has window W > 0 counts, per token, the codes its
//          last min(r, W) rows left in this column's ring (wave 0 copies them into s_rep ahead of the first barrier; every thread then
//          counts matches against its own tokens: in the vector path by comparisons unrolled over the 8 registers, never by indexing
//          them) and subtracts presence + frequency * count from the tokens it met, behind step 0 and ahead of step 1.  The thread that
//          stores tok32 and the code stores the code into ring slot r & 63 too, a forced workgroup included.  The record is
//          workgroup-uniform: a slot with W = 0 touches no ring and executes the arithmetic of the kernel without REP, operation for
//          operation.  REP = false compiles to what the body was before the flag existed.
//          W = 64: slot r & 63 holds row r - 64, the OLDEST entry read, and is the entry written.  The reads are wave 0's, ahead of the
//          barrier behind them; the store comes behind every barrier of the body, and a ring belongs to one workgroup of one launch.
//          (A forced workgroup without LP returns ahead of the barriers: it reads no entry at all.)
//   GUIDE  "guidance" (talkshow_hip.h): the slot's role is one uniform load ahead of everything else.  -2, a shadow: the workgroup
//          returns there, ahead of every load, store and barrier of the body; the condition depends on blockIdx alone, so the exit is
//          uniform over the workgroup and no wave waits at a barrier for one that left.  g >= 0, a primary: the row of slot g is read
//          through the strides of the slot's own row, l' = l + scale * (l - l_g) (guide_mix: three roundings) replaces l ahead of step
//          0 — in the vector path in the 8 registers, behind the row copies, which stay the network's two rows — and every store of the
//          slot's token, code, kept bytes and log-probability is made to slot g's entries as well; the ring read and written is the
//          slot's own.  -1: the arithmetic of the kernel without GUIDE, operation for operation.  GUIDE = false compiles to what the
//          body was before the flag existed.  Instantiated with BIAS = REP = true only.
//   ALT    "alternatives" (talkshow_hip.h): the row's n best allowed tokens with their log-probabilities, its entropy and the rank of its
//          code, all under the distribution of steps 1 and 2 (ahead of top-k and top-p), in the same launch.  The n best: n rounds of a
//          workgroup maximum over the tokens' packed places (alt_pack), each round over the tokens behind the round before it, so nothing
//          is marked as taken; a round's owner stores its d_j.  S_all and E: a second and a third chunk sum beside step 5's, added left to
//          right by one thread of wave 1 and one of wave 2 while thread 0 forms step 5's prefix sums.  The rank: the code's owner
//          publishes its packed place, every thread counts its tokens ahead of it, one integer LDS atomic per wave.  A forced workgroup
//          writes all four too.  Nothing here feeds the draw: idx and logprob are the bits of the kernel without ALT.  ALT = false
//          compiles to what the body was before the flag existed.  Instantiated with BIAS = REP = LP = true, GUIDE = false only.
// Inlined into its __global__ entries (eight without BIAS, eight with, eight with BIAS and REP, eight with GUIDE, four with ALT); DESIGN.md §5 ("One body per sampler
// family") records what was compared against the two separate kernel templates it replaces.
template <bool FAST, bool LP, bool GIVEN, bool BIAS = false, bool REP = false, bool GUIDE = false, bool ALT = false>
__device__ __forceinline__ void sample_ctl_body(const SampleCtlParams &cp, const int *rows, const int64_t *given, long given_stride,
                                                const unsigned char *keep, long keep_stride, float *sf, int *si, float &s_thr, int &s_last,
                                                uint32_t *s_tie, ctl_u64 (*hist)[256], int *s_rep = nullptr,
                                                const SampleAltParams *ap = nullptr, AltLds *al = nullptr) {
    const SampleParams &p = cp.s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(!GUIDE || (BIAS && REP), "the guided samplers imply the bias and repetition arithmetic");
    static_assert(!ALT || (BIAS && REP && LP && !GUIDE), "alternatives run on the most general unguided family");
    [[maybe_unused]] int gslot = -1;        // GUIDE: the shadow's slot of a primary, -1 for a plain slot
    [[maybe_unused]] float gscale = 0.f;
    if constexpr (GUIDE) {
        const int role = cp.guide_role[b];
        if (role == -2) return;             // a shadow draws nothing: out ahead of every barrier, the whole workgroup (blockIdx alone decides)
        if (role >= 0) {
            gslot = role;
            gscale = cp.guide_scale[b];
        }
    }
    const float *lg = sample_row(p, b);
    [[maybe_unused]] const float *lq = nullptr;   // GUIDE: the shadow's row, through the strides of the slot's own
    if constexpr (GUIDE) {
        if (gslot >= 0) lq = sample_row(p, gslot);
    }
    bool forced = false;       // workgroup-uniform, ahead of every barrier
    long long gcode = -1;
    if constexpr (GIVEN) {
        forced = given_forced(p, rows, keep, keep_stride, b);
        gcode = forced ? (long long)given[(long)b * given_stride] : -1;
    }

    const int chunk = (p.V + 255) / 256;
    const int v0 = tid * chunk, v1 = min(v0 + chunk, p.V);
    const int n = FAST ? 8 : max(v1 - v0, 0);
    float x[8];
    if constexpr (FAST) sample_load8(lg, v0, x);
    [[maybe_unused]] float xq[8];
    if constexpr (GUIDE && FAST) {
        if (lq) sample_load8(lq, v0, xq);
    }
    // BIAS: the clip's row of this column, or null (workgroup-uniform: the index is one uniform load)
    const float *bias = nullptr;
    if constexpr (BIAS) {
        const int t = cp.bias_index[b];
        if (t >= 0) bias = cp.bias + ((long)t * 2 + cp.bias_col) * p.V;
    }
    [[maybe_unused]] float xb[8];
    if constexpr (BIAS && FAST) {
        if (bias) sample_load8(bias, v0, xb);   // beside the logits: both pairs of loads are in flight ahead of the row copy
    }
    // REP: the clip's record (workgroup-uniform: one uniform load), its ring of this column, the launch's row r and the min(r - from_row, W)
    // entries to count (from_row: 0 in a one-shot pass; a session's row at which the clip's penalty was switched on, never above r).  The window is clamped to the ring: s_rep holds SAMPLE_REP_RING entries whatever a record says
    [[maybe_unused]] int rep_n = 0, rep_slot = 0;
    [[maybe_unused]] float rep_pres = 0.f, rep_freq = 0.f;
    [[maybe_unused]] int32_t *ring = nullptr;
    [[maybe_unused]] bool rep_any = false;     // generic path: one of this thread's tokens is in the window
    if constexpr (REP) {
        const SampleRep rr = cp.rep[b];
        if (rr.window > 0) {
            const uint32_t r = (p.position + (p.dyn ? (uint32_t)p.dyn[2] : 0u)) >> 1;
            ring = cp.rep_ring + ((long)b * 2 + cp.bias_col) * SAMPLE_REP_RING;
            rep_slot = (int)(r & (uint32_t)(SAMPLE_REP_RING - 1));
            rep_pres = rr.presence;
            rep_freq = rr.frequency;
            if (!(GIVEN && !LP && forced)) {   // rows r - 1, r - 2, ...: wave 0 alone (rep_n <= 64), ahead of the first barrier
                rep_n = (int)min(r - (uint32_t)rr.from_row, (uint32_t)min(rr.window, SAMPLE_REP_RING));
                if (tid < rep_n) s_rep[tid] = ring[(r - 1u - (uint32_t)tid) & (uint32_t)(SAMPLE_REP_RING - 1)];
            }
        }
    }
    auto rep_count = [&](int v) -> int {
        int c = 0;
        if constexpr (REP) {
            for (int i = 0; i < rep_n; ++i) c += s_rep[i] == v ? 1 : 0;
        }
        return c;
    };
    auto logit = [&](int k) -> float {
        if constexpr (FAST) return x[k];
        else if constexpr (REP) {
            float l = lg[v0 + k];
            if constexpr (GUIDE) {
                if (lq) l = guide_mix(l, lq[v0 + k], gscale);
            }
            if (bias) l = l + bias[v0 + k];
            return rep_any ? rep_penalise(l, rep_count(v0 + k), rep_pres, rep_freq) : l;
        }
        else if constexpr (BIAS) return bias ? lg[v0 + k] + bias[v0 + k] : lg[v0 + k];
        else return lg[v0 + k];
    };
    // BIAS: l' = -inf is out of the kept set whatever the record says (a neutral record included)
    auto banned = [&](int k) -> bool {
        if constexpr (BIAS) return bias && logit(k) == -INFINITY;
        else return false;
    };
    sample_copy_row(p, b, FAST, lg, x, v0, v1);   // the network's l: step 0 comes behind the copy
    if constexpr (GUIDE) {
        if (lq) {   // the shadow's row copy is the network's, too; then l' takes l's place
            sample_copy_row(p, gslot, FAST, lq, xq, v0, v1);
            if constexpr (FAST) {
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = guide_mix(x[k], xq[k], gscale);
            }
        }
    }
    // what a primary writes for itself it writes for its shadow (GUIDE; nothing otherwise)
    auto store_shadow = [&](int tok, long long code) {
        if constexpr (GUIDE) {
            if (gslot >= 0) {
                p.tok32[(long)gslot * p.tok_stride] = tok;
                p.codes[(long)gslot * p.code_stride] = code;
            }
        }
    };
    if constexpr (BIAS && FAST) {
        if (bias) {
#pragma unroll
            for (int k = 0; k < 8; ++k) x[k] = x[k] + xb[k];
        }
    }
    if constexpr (GIVEN && !LP) {
        if (forced) {
            if (tid == 0) {
                p.tok32[(long)b * p.tok_stride] = given_token(gcode, p.V);
                p.codes[(long)b * p.code_stride] = gcode;
                store_shadow(given_token(gcode, p.V), gcode);
                if constexpr (REP) {
                    if (ring) ring[rep_slot] = given_token(gcode, p.V);   // a taken code enters the history
                }
            }
            return;
        }
    }
    // REP, step 0b: l'' = l' - (presence + frequency * c) for the tokens the window met
    if constexpr (REP) {
        if (rep_n > 0) {   // workgroup-uniform
            __syncthreads();
            if constexpr (FAST) {
                int cnt[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) cnt[k] = 0;
                for (int i = 0; i < rep_n; ++i) {
                    const int d = s_rep[i] - v0;
                    if ((unsigned)d < 8u) {
#pragma unroll
                        for (int k = 0; k < 8; ++k) cnt[k] += d == k ? 1 : 0;
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) x[k] = rep_penalise(x[k], cnt[k], rep_pres, rep_freq);
            } else {
                for (int i = 0; i < rep_n; ++i) rep_any = rep_any || (s_rep[i] >= v0 && s_rep[i] < v1);
            }
        }
    }

    const SampleCtl rec = cp.ctl[b];
    CtlSel S;
    S.need_k = rec.top_k >= 1 && rec.top_k < p.V;
    S.need_p = rec.top_p < 1.0f;
    const bool sel = S.need_k || S.need_p;   // workgroup-uniform: a neutral record (and a temperature alone) goes straight to the draw
    if (sel) {
#pragma unroll
        for (int i = 0; i < 7; ++i) hist[i][tid] = 0;
    }

    // ---- max / argmax as in the plain body; ties -> lowest index ----
    float best = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll 8
    for (int k = 0; k < n; ++k) {
        const float t = logit(k);
        if (t > best) { best = t; bi = v0 + k; }
    }
    sample_argmax(best, bi, sf, si);

    // the uniform: the plain body's source, so it does not depend on the record; a forced row reads none
    float u = 0.f;
    if (!forced) u = sample_uniform(p, b);

    const float inv_t = rec.inv_t;
    auto weight = [&](int k) -> float { return ctl_weight(logit(k), best, inv_t); };

    // ---- steps 2-4: the kept set ----
    uint32_t key[8], q[8];
    auto key_of = [&](int k) -> uint32_t {
        if constexpr (FAST) return key[k];
        else return ctl_key(logit(k));
    };
    auto q_of = [&](int k) -> uint32_t {
        if constexpr (FAST) return q[k];
        else return ctl_quant(weight(k));
    };
    int jk0 = 0, jp0 = 0;
    if (sel) {
        if constexpr (FAST) {
#pragma unroll
            for (int k = 0; k < 8; ++k) { key[k] = ctl_key(x[k]); q[k] = ctl_quant(weight(k)); }
        }
        // level lv of a descent: the tokens whose upper 8 lv key bits equal `prefix`, binned by the next 8
        auto fill = [&](ctl_u64 *h, int lv, uint32_t prefix) {
#pragma unroll 8
            for (int k = 0; k < n; ++k) {
                const uint32_t ky = key_of(k);
                if (lv == 0 || (ky >> (32 - 8 * lv)) == prefix)
                    atomicAdd(&h[(ky >> (24 - 8 * lv)) & 255u], (1ull << CTL_CNT_SHIFT) | (ctl_u64)q_of(k));
            }
            __syncthreads();
        };
        fill(hist[0], 0, 0u);
        ctl_u64 Qk;   // quantised mass of the tokens top-k keeps
        if (S.need_k) {
            uint32_t prefix = 0;
            ctl_u64 acc = 0;
            for (int lv = 0; lv < 4; ++lv) {
                if (lv > 0) fill(hist[lv], lv, prefix);
                prefix = (prefix << 8) | (uint32_t)(ctl_pick_bin(hist[lv], lane, false, (ctl_u64)rec.top_k, acc) & 255);
            }
            S.Kk = prefix;
            S.ntie_k = rec.top_k - (int)(acc >> CTL_CNT_SHIFT);
            Qk = (acc & CTL_MASS_MASK) + (ctl_u64)S.ntie_k * ctl_quant(ctl_weight(ctl_unkey(prefix), best, inv_t));   // equal logits, equal weights
        } else {
            S.Kk = 0;
            S.ntie_k = 0;
            Qk = ctl_hist_total(hist[0], lane) & CTL_MASS_MASK;
        }
        S.Kp = 0; S.p_top = false; S.mgt_p = S.q_p = S.Tq = 0;
        if (S.need_p) {
            S.Tq = (ctl_u64)ceil((double)rec.top_p * (double)Qk);   // M < p * Qk  <=>  M < ceil(p * Qk) for an integer M; one fp64 product
            uint32_t prefix = 0;
            ctl_u64 acc = 0;
            for (int lv = 0; lv < 4; ++lv) {
                ctl_u64 *h = lv == 0 ? hist[0] : hist[3 + lv];
                if (lv > 0) fill(h, lv, prefix);
                prefix = (prefix << 8) | (uint32_t)(ctl_pick_bin(h, lane, true, S.Tq, acc) & 255);
            }
            S.Kp = prefix;
            S.mgt_p = acc & CTL_MASS_MASK;
            S.p_top = (acc >> CTL_CNT_SHIFT) == 0;
            S.q_p = ctl_quant(ctl_weight(ctl_unkey(prefix), best, inv_t));
        }
        // ties at the boundary keys owned by lower threads (= lower indices): one packed exclusive prefix count (both counts < 2^16)
        uint32_t c = 0;
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            const uint32_t ky = key_of(k);
            c += (S.need_k && ky == S.Kk ? 1u : 0u) + (S.need_p && ky == S.Kp ? 65536u : 0u);
        }
        uint32_t inc = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == 63) s_tie[wave] = inc;
        __syncthreads();
        uint32_t ex = inc - c;
        for (int w = 0; w < wave; ++w) ex += s_tie[w];
        jk0 = (int)(ex & 0xffffu);
        jp0 = (int)(ex >> 16);
    }

    // ---- ALT: the n best allowed tokens of step 2's ranking, one workgroup maximum per round ----
    if constexpr (ALT) {
        if (tid == 0) { al->ck = 0; al->rank = 0; }   // read behind later barriers only
        ctl_u64 prev = ~0ull;                         // the place taken by the round before: this round looks behind it
        for (int j = 0; j < ap->n; ++j) {             // workgroup-uniform
            ctl_u64 mb = 0;
            float ml = 0.f;
#pragma unroll 8
            for (int k = 0; k < n; ++k) {
                const float l = logit(k);
                const ctl_u64 pk = alt_pack(ctl_key(l), v0 + k);
                if (l != -INFINITY && pk < prev && pk > mb) { mb = pk; ml = l; }
            }
            ctl_u64 wb = mb;
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const ctl_u64 o = __shfl_xor(wb, off);
                wb = o > wb ? o : wb;
            }
            if (lane == 0) al->top[j & 1][wave] = wb;
            __syncthreads();
            ctl_u64 win = al->top[j & 1][0];
            for (int w = 1; w < 4; ++w) win = al->top[j & 1][w] > win ? al->top[j & 1][w] : win;
            if (tid == 0) al->code[j] = win ? alt_index(win) : -1;   // 0: fewer allowed tokens than n
            if (win && mb == win) al->d[j] = ctl_arg(ml, best, inv_t);   // the owner: a place holds its index, so there is one
            prev = win;
        }
    }

    // ---- step 5: the plain body's inverse CDF over w' = kept ? w : 0 (adding a zero changes no bit, so dropped tokens are skipped);
    //      the owner of a given code notes its logit and whether it was kept ----
    float s = 0.f;
    int hi = -1;   // highest kept index of the chunk
    [[maybe_unused]] AltSums<ALT> asum;
    bool gkept = false;
    float glc = 0.f;
    {
        int jk = jk0, jp = jp0;
        unsigned char *kd = cp.kept ? cp.kept + (long)b * p.V : nullptr;
        [[maybe_unused]] unsigned char *kq = nullptr;
        if constexpr (GUIDE) {
            if (cp.kept && gslot >= 0) kq = cp.kept + (long)gslot * p.V;
        }
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            bool kp = !sel || ctl_keep(S, key_of(k), jk, jp);
            if constexpr (BIAS) kp = kp && !banned(k);
            if (kp) { s += weight(k); hi = v0 + k; }
            if (kd) kd[v0 + k] = kp ? 1 : 0;
            if constexpr (GUIDE) {
                if (kq) kq[v0 + k] = kp ? 1 : 0;
            }
            if constexpr (GIVEN && LP) {
                if ((long long)(v0 + k) == gcode) { gkept = kp; glc = logit(k); }
            }
            if constexpr (ALT) {   // every token with l'' above -inf, whatever the filters keep
                const float l = logit(k);
                if (l != -INFINITY) {
                    const float d = ctl_arg(l, best, inv_t);
                    const float w = det_expf(d);
                    asum.s += w;
                    if (w > 0.f) asum.e = alt_acc(asum.e, w, d);
                }
            }
        }
    }
    sf[tid + 1] = s;
    si[tid] = hi;
    if constexpr (ALT) { al->sa[tid] = asum.s; al->se[tid] = asum.e; }
    __syncthreads();
    if (tid == 0) {
        s_thr = u * sample_prefix_sum<true>(sf, si, &s_last);   // s_last: the highest kept index of the row (rank 0 is always kept)
    }
    if constexpr (ALT) {   // the chunk sums left to right, beside thread 0's
        if (tid == 64 || tid == 128) {
            const float *src = tid == 64 ? al->sa : al->se;
            float c = 0.f;
            for (int t = 0; t < 256; ++t) c += src[t];
            al->tot[tid == 64 ? 0 : 1] = c;
        }
    }
    __syncthreads();
    if constexpr (GIVEN && LP) {
        if (forced) {   // workgroup-uniform: S = sf[256] is there, nothing is drawn
            float *out = cp.logprob + (long)b * cp.lp_stride;
            if constexpr (GUIDE) {
                float *outq = gslot >= 0 ? cp.logprob + (long)gslot * cp.lp_stride : nullptr;
                if (gcode >= (long long)v0 && gcode < (long long)v1) {
                    const float val = sample_logprob_value(ctl_arg(glc, best, inv_t), sf[256], gkept);
                    *out = val;
                    if (outq) *outq = val;
                }
                if (tid == 0 && outq) sample_store_unowned(outq, gcode, p.V);
            } else {
                if (gcode >= (long long)v0 && gcode < (long long)v1) sample_store_logprob(out, ctl_arg(glc, best, inv_t), sf[256], gkept);
            }
            if (tid == 0) {
                sample_store_unowned(out, gcode, p.V);
                p.tok32[(long)b * p.tok_stride] = given_token(gcode, p.V);
                p.codes[(long)b * p.code_stride] = gcode;
                store_shadow(given_token(gcode, p.V), gcode);
                if constexpr (REP) {
                    if (ring) ring[rep_slot] = given_token(gcode, p.V);
                }
            }
            if constexpr (ALT) alt_finish(ap, al, gcode, b, v0, v1, n, logit);
            return;
        }
    }
    const float thr = s_thr;
    const bool mine = (sf[tid] <= thr) && (thr < sf[tid + 1] || tid == 255);
    const int last = s_last;
    __syncthreads();   // si[0] becomes the result below: every thread has read what it needs
    if (mine) {
        int res = -1;
        float c = sf[tid];
        int jk = jk0, jp = jp0;
#pragma unroll 8
        for (int k = 0; k < n; ++k) {
            bool kp = !sel || ctl_keep(S, key_of(k), jk, jp);
            if constexpr (BIAS) kp = kp && !banned(k);
            if (kp) {
                c += weight(k);
                if (res < 0 && c > thr) res = v0 + k;   // the first crossing is latched
            }
        }
        // no crossing: inside an owning chunk its highest kept token; with no running sum above u * total (u = 1 - 2^-24) the row's
        if (res < 0) res = (thr < sf[tid + 1] && hi >= 0) ? hi : last;
        si[0] = res;
    }
    __syncthreads();
    if (tid == 0) {
        const int choice = si[0];
        p.tok32[(long)b * p.tok_stride] = choice;
        p.codes[(long)b * p.code_stride] = choice;
        store_shadow(choice, choice);
        if constexpr (REP) {
            if (ring) ring[rep_slot] = choice;
        }
    }
    if constexpr (LP) {
        const int choice = si[0];
        if (choice >= v0 && choice < v1) {   // the owner of the drawn index (a draw is always a kept token of the row)
            float lc = 0.f;
#pragma unroll 8
            for (int k = 0; k < n; ++k)
                if (v0 + k == choice) lc = logit(k);
            if constexpr (GUIDE) {
                const float val = sample_logprob_value(ctl_arg(lc, best, inv_t), sf[256]);
                cp.logprob[(long)b * cp.lp_stride] = val;
                if (gslot >= 0) cp.logprob[(long)gslot * cp.lp_stride] = val;
            } else {
                sample_store_logprob(cp.logprob + (long)b * cp.lp_stride, ctl_arg(lc, best, inv_t), sf[256]);
            }
        }
    }
    if constexpr (ALT) alt_finish(ap, al, (long long)si[0], b, v0, v1, n, logit);
}

template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_kernel(const SampleCtlParams cp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];   // levels 0-3 of the top-k descent (level 0 shared), 1-3 of the top-p descent
    sample_ctl_body<FAST, LP, false>(cp, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr, s_last, s_tie, hist);
}
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, true>(gp.c, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si, s_thr, s_last, s_tie, hist);
}

// "code bias": the same two entry families with BIAS = true, launched only for a run that brings tables (p.bias != null)
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_bias_kernel(const SampleCtlParams cp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, false, true>(cp, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr, s_last, s_tie, hist);
}
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_bias_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, true, true>(gp.c, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si, s_thr, s_last, s_tie, hist);
}
// "repetition penalty": the two families once more with BIAS = true and REP = true, launched only for a run that brings records
// (p.rep != null).  A run without tables brings an index of -1 everywhere, which the BIAS path treats as "no table, same arithmetic"
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_rep_kernel(const SampleCtlParams cp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, false, true, true>(cp, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr, s_last, s_tie, hist, s_rep);
}
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_rep_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, true, true, true>(gp.c, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si, s_thr, s_last, s_tie, hist,
                                                s_rep);
}
// "guidance": the two families once more with BIAS = REP = GUIDE = true, launched only for a run that brings a role table
// (p.guide_role != null).  A run without records brings records of window 0, one without tables an index of -1 everywhere
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_guide_kernel(const SampleCtlParams cp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, false, true, true, true>(cp, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr, s_last, s_tie, hist, s_rep);
}
template <bool FAST, bool LP>
__global__ __launch_bounds__(256) void sample_ctl_guide_given_kernel(const SampleGivenParams gp) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, LP, true, true, true, true>(gp.c, gp.rows, gp.given, gp.given_stride, gp.keep, gp.keep_stride, sf, si, s_thr, s_last, s_tie,
                                                      hist, s_rep);
}
// "alternatives": the family with BIAS = REP = LP = true once more with ALT = true, launched only for a run that asks for alternatives.
// A run without records brings records of window 0, one without tables an index of -1 everywhere, one without a table neutral records
template <bool FAST>
__global__ __launch_bounds__(256) void sample_ctl_alt_kernel(const SampleAltParams ap) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ AltLds al;
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, true, false, true, true, false, true>(ap.g.c, nullptr, nullptr, 0, nullptr, 0, sf, si, s_thr, s_last, s_tie, hist, s_rep, &ap,
                                                                &al);
}
template <bool FAST>
__global__ __launch_bounds__(256) void sample_ctl_alt_given_kernel(const SampleAltParams ap) {
    __shared__ float sf[256 + 1];
    __shared__ int si[256];
    __shared__ float s_thr;
    __shared__ int s_last;
    __shared__ uint32_t s_tie[4];
    __shared__ int s_rep[SAMPLE_REP_RING];
    __shared__ AltLds al;
    __shared__ __attribute__((aligned(16))) ctl_u64 hist[7][256];
    sample_ctl_body<FAST, true, true, true, true, false, true>(ap.g.c, ap.g.rows, ap.g.given, ap.g.given_stride, ap.g.keep, ap.g.keep_stride, sf, si,
                                                               s_thr, s_last, s_tie, hist, s_rep, &ap, &al);
}
// rows at or beyond a clip's own H_b: -1, 0, 0, -1 (one thread per position; beside mask_logprob_kernel)
__global__ void mask_alt_kernel(int32_t *codes, float *logprob, float *entropy, int32_t *rank, int n, int B, int H, const int *__restrict__ lens) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * H * 2) return;
    const int b = (int)(i / ((long)H * 2)), r = (int)((i / 2) % H);
    if (r < (lens[b] >> 2)) return;
    for (int j = 0; j < n; ++j) { codes[i * n + j] = -1; logprob[i * n + j] = 0.f; }
    entropy[i] = 0.f;
    rank[i] = -1;
}
hipError_t launch_mask_alt(int32_t *codes, float *logprob, float *entropy, int32_t *rank, int n, int B, int H, const int *lens, hipStream_t stream) {
    if (!entropy || !rank || !lens || B < 1 || H < 1 || n < 0 || n > SAMPLE_ALT_MAX || (n > 0 && (!codes || !logprob))) return hipErrorInvalidValue;
    const long total = (long)B * H * 2;
    hipLaunchKernelGGL(mask_alt_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, codes, logprob, entropy, rank, n, B, H, lens);
    return hipGetLastError();
}

// what a launch with tables needs beyond its sibling's checks; the vector path also needs 16-byte aligned table rows (V = 2048: every row
// of an aligned block is)
static bool sample_bias_ok(const SampleCtlParams &p) { return p.ctl && p.bias_index && (p.bias_col == 0 || p.bias_col == 1); }
static bool sample_bias_fast(const SampleCtlParams &p) { return (reinterpret_cast<uintptr_t>(p.bias) & 15) == 0; }
// and a launch with records: its ring, and the index table the BIAS path reads (tables themselves are optional)
static bool sample_rep_ok(const SampleCtlParams &p) { return p.ctl && p.rep_ring && p.bias_index && (p.bias_col == 0 || p.bias_col == 1); }
// and a guided launch: the scale table, and what the REP path reads (records of window 0 where the run brought none)
static bool sample_guide_ok(const SampleCtlParams &p) { return p.guide_scale && p.rep && sample_rep_ok(p); }

hipError_t launch_sample_ctl(const SampleCtlParams &p, hipStream_t stream) {
    if (!p.ctl || p.s.V < 1 || p.s.V > SAMPLE_CTL_MAX_V || (p.s.mode != TS_SAMPLE_UNIFORMS && p.s.mode != TS_SAMPLE_PHILOX)) return hipErrorInvalidValue;
    const long ls = p.s.logit_stride ? p.s.logit_stride : (long)p.s.V;
    const bool fast = p.s.V == 2048 && (ls & 3) == 0 && (reinterpret_cast<uintptr_t>(p.s.logits) & 15) == 0;
    if (p.guide_role) {
        if (!sample_guide_ok(p)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p);
        if (p.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_guide_kernel<true, true>), dim3(p.s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_guide_kernel<false, true>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_guide_kernel<true, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_guide_kernel<false, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.rep) {
        if (!sample_rep_ok(p)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p);
        if (p.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_rep_kernel<true, true>), dim3(p.s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_rep_kernel<false, true>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_rep_kernel<true, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_rep_kernel<false, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.bias) {
        if (!sample_bias_ok(p)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p);
        if (p.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_bias_kernel<true, true>), dim3(p.s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_bias_kernel<false, true>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_bias_kernel<true, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_bias_kernel<false, false>), dim3(p.s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.logprob) {
        if (fast) hipLaunchKernelGGL((sample_ctl_kernel<true, true>), dim3(p.s.B), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((sample_ctl_kernel<false, true>), dim3(p.s.B), dim3(256), 0, stream, p);
    } else if (fast) {
        hipLaunchKernelGGL((sample_ctl_kernel<true, false>), dim3(p.s.B), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL((sample_ctl_kernel<false, false>), dim3(p.s.B), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_sample_given(const SampleGivenParams &p, hipStream_t stream) {
    const SampleParams &s = p.c.s;
    if (!p.rows || !p.given || s.V < 1) return hipErrorInvalidValue;
    if (s.mode != TS_SAMPLE_GREEDY && s.mode != TS_SAMPLE_UNIFORMS && s.mode != TS_SAMPLE_PHILOX) return hipErrorInvalidValue;
    if (!p.c.ctl) {
        if (p.c.kept || p.c.bias || p.c.rep || p.c.guide_role) return hipErrorInvalidValue;
        if (p.c.logprob) hipLaunchKernelGGL(sample_lp_given_kernel, dim3(s.B), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL(sample_given_kernel, dim3(s.B), dim3(256), 0, stream, p);
        return hipGetLastError();
    }
    if (s.V > SAMPLE_CTL_MAX_V || s.mode == TS_SAMPLE_GREEDY) return hipErrorInvalidValue;
    const long ls = s.logit_stride ? s.logit_stride : (long)s.V;
    const bool fast = s.V == 2048 && (ls & 3) == 0 && (reinterpret_cast<uintptr_t>(s.logits) & 15) == 0;
    if (p.c.guide_role) {
        if (!sample_guide_ok(p.c)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p.c);
        if (p.c.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_guide_given_kernel<true, true>), dim3(s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_guide_given_kernel<false, true>), dim3(s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_guide_given_kernel<true, false>), dim3(s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_guide_given_kernel<false, false>), dim3(s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.c.rep) {
        if (!sample_rep_ok(p.c)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p.c);
        if (p.c.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_rep_given_kernel<true, true>), dim3(s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_rep_given_kernel<false, true>), dim3(s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_rep_given_kernel<true, false>), dim3(s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_rep_given_kernel<false, false>), dim3(s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.c.bias) {
        if (!sample_bias_ok(p.c)) return hipErrorInvalidValue;
        const bool bfast = fast && sample_bias_fast(p.c);
        if (p.c.logprob) {
            if (bfast) hipLaunchKernelGGL((sample_ctl_bias_given_kernel<true, true>), dim3(s.B), dim3(256), 0, stream, p);
            else hipLaunchKernelGGL((sample_ctl_bias_given_kernel<false, true>), dim3(s.B), dim3(256), 0, stream, p);
        } else if (bfast) {
            hipLaunchKernelGGL((sample_ctl_bias_given_kernel<true, false>), dim3(s.B), dim3(256), 0, stream, p);
        } else {
            hipLaunchKernelGGL((sample_ctl_bias_given_kernel<false, false>), dim3(s.B), dim3(256), 0, stream, p);
        }
        return hipGetLastError();
    }
    if (p.c.logprob) {
        if (fast) hipLaunchKernelGGL((sample_ctl_given_kernel<true, true>), dim3(s.B), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((sample_ctl_given_kernel<false, true>), dim3(s.B), dim3(256), 0, stream, p);
    } else if (fast) {
        hipLaunchKernelGGL((sample_ctl_given_kernel<true, false>), dim3(s.B), dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL((sample_ctl_given_kernel<false, false>), dim3(s.B), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

hipError_t launch_sample_alt(const SampleAltParams &p, hipStream_t stream) {
    const SampleCtlParams &c = p.g.c;
    const SampleParams &s = c.s;
    if (s.V < 1 || s.V > SAMPLE_CTL_MAX_V || (s.mode != TS_SAMPLE_UNIFORMS && s.mode != TS_SAMPLE_PHILOX)) return hipErrorInvalidValue;
    if (!c.logprob || !c.rep || c.guide_role || !sample_rep_ok(c)) return hipErrorInvalidValue;
    if (p.n < 0 || p.n > SAMPLE_ALT_MAX || !p.entropy || !p.rank || (p.n > 0 && (!p.codes || !p.logprob))) return hipErrorInvalidValue;
    if (p.g.rows && !p.g.given) return hipErrorInvalidValue;
    const long ls = s.logit_stride ? s.logit_stride : (long)s.V;
    const bool fast = s.V == 2048 && (ls & 3) == 0 && (reinterpret_cast<uintptr_t>(s.logits) & 15) == 0 && sample_bias_fast(c);
    if (p.g.rows) {
        if (fast) hipLaunchKernelGGL((sample_ctl_alt_given_kernel<true>), dim3(s.B), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((sample_ctl_alt_given_kernel<false>), dim3(s.B), dim3(256), 0, stream, p);
    } else {
        if (fast) hipLaunchKernelGGL((sample_ctl_alt_kernel<true>), dim3(s.B), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((sample_ctl_alt_kernel<false>), dim3(s.B), dim3(256), 0, stream, p);
    }
    return hipGetLastError();
}

}  // namespace ts
