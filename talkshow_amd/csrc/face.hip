// Kernels of the face generator that are not GEMM-shaped (everything GEMM-shaped runs on conv_gemm_f32):
//   w2v_conv0_*      wav2vec2 feature-extractor layer 0: Conv1d(1,512,k10,s5,no bias) + GroupNorm(512,512) + GELU
//                    (HF Wav2Vec2GroupNormConvLayer; called at nets/spg/wav2vec.py:92).  Bandwidth bound: the conv is
//                    computed in the apply pass (10 MAC/output) and never stored un-normalised; the GroupNorm statistics
//                    come from the waveform's second moments (65 sums per clip), not from a pass over the 512 channels.
//   lerp_ln          linear_interpolation 50->30 fps (nets/spg/wav2vec.py:64-70) fused with the feature-projection
//                    LayerNorm(512) (HF Wav2Vec2FeatureProjection; :107)
//   layernorm_rows   nn.LayerNorm over channels (+ post-norm residual, ReLU): encoder LNs and nets/layers.py:142-151
//   attention        fused QK^T -> online soft-max -> PV of HF eager_attention_forward, one workgroup per 64 queries of a (clip, head)
//   fill_id          id_mlp(one-hot id) broadcast over time and concatenated (nets/spg/s2g_face.py:127-130)
#include <cstring>

#include "kernels.h"

namespace ts {

constexpr int C0_TB = 128;   // output frames per block in the conv0 kernels

__device__ inline float gelu_erf(float v) { return gelu_fast(v); }   // kernels.h: libm's erf algorithm, branch-free

// partial sums of conv0 output per (clip, time block, channel): grid (tblocks, B), 256 threads x 2 channels
__global__ __launch_bounds__(256) void w2v_conv0_stats_kernel(const float *__restrict__ wav, int N, int L0,
                                                              const float *__restrict__ w, double2 *__restrict__ part,
                                                              int C) {
    __shared__ float sw[C0_TB * 5 + 16];
    const int b = blockIdx.y, tb = blockIdx.x, t0 = tb * C0_TB;
    const int nt = min(C0_TB, L0 - t0);
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < N ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) wk[k] = w[c * 10 + k];
        double s = 0.0, s2 = 0.0;
        for (int t = 0; t < nt; ++t) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) v = fmaf(wk[k], sw[t * 5 + k], v);
            s += v;
            s2 += (double)v * v;
        }
        part[((long)b * gridDim.x + tb) * C + c] = double2{s, s2};
    }
}

// fixed-order reduction over the time blocks -> (mean, rstd) per (clip, channel)
__global__ void w2v_gn_finalize_kernel(const double2 *__restrict__ part, int ntb, int C, int L0, float2 *__restrict__ stats,
                                       int BC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    double s = 0.0, s2 = 0.0;
    for (int t = 0; t < ntb; ++t) {
        const double2 v = part[((long)b * ntb + t) * C + c];
        s += v.x;
        s2 += v.y;
    }
    const double mean = s / L0;
    double var = s2 / L0 - mean * mean;
    if (var < 0) var = 0;
    stats[i] = float2{(float)mean, (float)(1.0 / sqrt(var + 1e-5))};
}

// recompute conv0, normalise, GELU, store NLC (B, L0, C)
__global__ __launch_bounds__(256) void w2v_conv0_apply_kernel(const float *__restrict__ wav, int N, int L0,
                                                              const float *__restrict__ w, const float2 *__restrict__ stats,
                                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                                              float *__restrict__ out, int C) {
    __shared__ float sw[C0_TB * 5 + 16];
    const int b = blockIdx.y, t0 = blockIdx.x * C0_TB;
    const int nt = min(C0_TB, L0 - t0);
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < N ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) wk[k] = w[c * 10 + k];
        const float2 st = stats[b * C + c];
        const float g = gamma[c], be = beta[c];
        for (int t = 0; t < nt; ++t) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) v = fmaf(wk[k], sw[t * 5 + k], v);
            v = (v - st.x) * st.y * g + be;
            out[((long)b * L0 + t0 + t) * C + c] = gelu_erf(v);
        }
    }
}

// ---- the same statistics from the input's second moments.  conv0's output is linear in its 10-sample window: y_c[t] = sum_k w[c][k] x[5 t + k],
// so over a clip  sum_t y_c = sum_k w[c][k] S[k]  and  sum_t y_c^2 = sum_{k,k'} w[c][k] w[c][k'] R[k][k']  with S[k] = sum_t x[5 t + k] and
// R[k][k'] = sum_t x[5 t + k] x[5 t + k'] — 65 numbers per clip (10 + 55, R is symmetric) instead of 512 x 2, and one pass over the waveform that
// does 65 products per frame instead of 5 120 MACs.  Products of two floats are exact in double and all sums run in double in a fixed order: the
// statistics are those of the exact convolution (the fp32 rounding of y in the direct form moves them by ~1e-8 relative; tests bound the face
// generator against the reference either way).  Statistics pass 0.47 -> 0.07 ms per face batch of 64 (56 + 9.5 + 4.7 us for the three kernels). ----
constexpr int C0_MB = 1024;                 // frames per block of the moments kernel (20 KB of LDS: seven blocks per CU)
constexpr int C0_NQ = 65;                   // S[0..9], then R[k][k'] for k <= k' row by row
__global__ __launch_bounds__(256) void w2v_conv0_moments_kernel(const float *__restrict__ wav, int N, int L0, double *__restrict__ part) {
    __shared__ float sw[C0_MB * 5 + 16];
    __shared__ double red[3][C0_NQ];
    const int b = blockIdx.y, t0 = blockIdx.x * C0_MB;
    const int nt = min(C0_MB, L0 - t0);
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < N ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    const int q = threadIdx.x % C0_NQ, slice = threadIdx.x / C0_NQ;   // 195 threads: quantity q over every third frame
    if (slice < 3) {
        int k = q, k2 = -1;                 // q < 10: S[q]
        if (q >= 10) {                      // pair number q - 10 in the order (0,0) (0,1) .. (0,9) (1,1) ..
            int r = q - 10;
            k = 0;
            while (r >= 10 - k) {
                r -= 10 - k;
                ++k;
            }
            k2 = k + r;
        }
        // eight independent partial sums: the loop is a chain of LDS round trips + one dependent double add otherwise (3 waves per SIMD)
        const float *pa = sw + k, *pb = k2 < 0 ? nullptr : sw + k2;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int t = slice;
        for (; t + 21 < nt; t += 24) {
            float va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                va[u] = pa[(t + 3 * u) * 5];
                vb[u] = pb ? pb[(t + 3 * u) * 5] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += (double)va[u] * (double)vb[u];
        }
        for (; t < nt; t += 3) acc[0] += (double)pa[t * 5] * (pb ? (double)pb[t * 5] : 1.0);
        red[slice][q] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    __syncthreads();
    if (threadIdx.x < C0_NQ) part[((long)b * gridDim.x + blockIdx.x) * C0_NQ + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x];
}

// fixed-order sum over the blocks of a clip -> mom[b][65]
__global__ void w2v_moments_reduce_kernel(const double *__restrict__ part, int nblk, double *__restrict__ mom, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int b = i / C0_NQ, q = i - b * C0_NQ;
    double s = 0.0;
    for (int t = 0; t < nblk; ++t) s += part[((long)b * nblk + t) * C0_NQ + q];
    mom[i] = s;
}

// (mean, rstd) of channel c of clip b from the clip's moments
__global__ void w2v_gn_from_moments_kernel(const double *__restrict__ mom, const float *__restrict__ w, int C, int L0, float2 *__restrict__ stats, int BC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    const double *m = mom + (long)b * C0_NQ;
    double wk[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) wk[k] = (double)w[c * 10 + k];
    double s = 0.0, s2 = 0.0;
    int q = 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        s += wk[k] * m[k];
#pragma unroll
        for (int k2 = k; k2 < 10; ++k2, ++q) s2 += (k2 == k ? 1.0 : 2.0) * wk[k] * wk[k2] * m[q];
    }
    const double mean = s / L0;
    double var = s2 / L0 - mean * mean;
    if (var < 0) var = 0;
    stats[i] = float2{(float)mean, (float)(1.0 / sqrt(var + 1e-5))};
}

hipError_t launch_w2v_conv0(const float *wav, int B, int N, int L0, const float *w, const float *gamma, const float *beta,
                            double2 *part, float2 *stats, float *out, int C, bool moments, hipStream_t s) {
    const int ntb = (L0 + C0_TB - 1) / C0_TB;
    if (moments) {   // `part` holds B x ntb x C double2: room for B x nblk x 65 + B x 65 doubles many times over
        const int nblk = (L0 + C0_MB - 1) / C0_MB;
        double *pm = reinterpret_cast<double *>(part), *mom = pm + (size_t)B * nblk * C0_NQ;
        hipLaunchKernelGGL(w2v_conv0_moments_kernel, dim3(nblk, B), dim3(256), 0, s, wav, N, L0, pm);
        hipLaunchKernelGGL(w2v_moments_reduce_kernel, dim3((B * C0_NQ + 255) / 256), dim3(256), 0, s, pm, nblk, mom, B * C0_NQ);
        hipLaunchKernelGGL(w2v_gn_from_moments_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, mom, w, C, L0, stats, B * C);
    } else {
        hipLaunchKernelGGL(w2v_conv0_stats_kernel, dim3(ntb, B), dim3(256), 0, s, wav, N, L0, w, part, C);
        hipLaunchKernelGGL(w2v_gn_finalize_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, ntb, C, L0, stats, B * C);
    }
    hipLaunchKernelGGL(w2v_conv0_apply_kernel, dim3(ntb, B), dim3(256), 0, s, wav, N, L0, w, stats, gamma, beta, out, C);
    return hipGetLastError();
}

// ---- length variants of the conv0 kernels (mixed passes: clips of different lengths padded to N samples; ns = the clips' own sample counts on the
// device).  The statements of the kernels above on the clip's own counts: a clip's frames fall into the same time blocks as when it runs alone,
// blocks beyond its last frame add exact zeros to the fixed-order double sums, no sample at or beyond ns[b] is read, and the apply pass stores
// zeros for the rows between the clip's own count and the padded one.  Kernels of their own: the uniform ones keep their names and their code ----
__host__ __device__ inline int w2v_l0(int n) { return (n - 10) / 5 + 1; }
__global__ __launch_bounds__(256) void w2v_conv0_stats_len_kernel(const float *__restrict__ wav, int N, const int *__restrict__ ns,
                                                              const float *__restrict__ w, double2 *__restrict__ part,
                                                              int C) {
    __shared__ float sw[C0_TB * 5 + 16];
    const int b = blockIdx.y, tb = blockIdx.x, t0 = tb * C0_TB;
    const int n = ns[b], L0 = w2v_l0(n);
    const int nt = min(C0_TB, L0 - t0);   // <= 0 in a block beyond the clip: every loop below is empty, the block's sums are exact zeros
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < n ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) wk[k] = w[c * 10 + k];
        double s = 0.0, s2 = 0.0;
        for (int t = 0; t < nt; ++t) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) v = fmaf(wk[k], sw[t * 5 + k], v);
            s += v;
            s2 += (double)v * v;
        }
        part[((long)b * gridDim.x + tb) * C + c] = double2{s, s2};
    }
}
__global__ void w2v_gn_finalize_len_kernel(const double2 *__restrict__ part, int ntb, int C, const int *__restrict__ ns, float2 *__restrict__ stats,
                                       int BC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    const int L0 = w2v_l0(ns[b]);
    double s = 0.0, s2 = 0.0;
    for (int t = 0; t < ntb; ++t) {
        const double2 v = part[((long)b * ntb + t) * C + c];
        s += v.x;
        s2 += v.y;
    }
    const double mean = s / L0;
    double var = s2 / L0 - mean * mean;
    if (var < 0) var = 0;
    stats[i] = float2{(float)mean, (float)(1.0 / sqrt(var + 1e-5))};
}
__global__ __launch_bounds__(256) void w2v_conv0_apply_len_kernel(const float *__restrict__ wav, int N, int L0, const int *__restrict__ ns,
                                                              const float *__restrict__ w, const float2 *__restrict__ stats,
                                                              const float *__restrict__ gamma, const float *__restrict__ beta,
                                                              float *__restrict__ out, int C) {
    __shared__ float sw[C0_TB * 5 + 16];
    const int b = blockIdx.y, t0 = blockIdx.x * C0_TB;
    const int n = ns[b];
    const int nt = min(C0_TB, w2v_l0(n) - t0);   // the clip's own rows of this block (L0 = the padded clip's: the pitch of `out`)
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < n ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) wk[k] = w[c * 10 + k];
        const float2 st = stats[b * C + c];
        const float g = gamma[c], be = beta[c];
        for (int t = 0; t < nt; ++t) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) v = fmaf(wk[k], sw[t * 5 + k], v);
            v = (v - st.x) * st.y * g + be;
            out[((long)b * L0 + t0 + t) * C + c] = gelu_erf(v);
        }
        for (int t = max(nt, 0); t < min(C0_TB, L0 - t0); ++t) out[((long)b * L0 + t0 + t) * C + c] = 0.f;
    }
}
__global__ __launch_bounds__(256) void w2v_conv0_moments_len_kernel(const float *__restrict__ wav, int N, const int *__restrict__ ns, double *__restrict__ part) {
    __shared__ float sw[C0_MB * 5 + 16];
    __shared__ double red[3][C0_NQ];
    const int b = blockIdx.y, t0 = blockIdx.x * C0_MB;
    const int n = ns[b];
    const int nt = min(C0_MB, w2v_l0(n) - t0);
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < n ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    const int q = threadIdx.x % C0_NQ, slice = threadIdx.x / C0_NQ;   // 195 threads: quantity q over every third frame
    if (slice < 3) {
        int k = q, k2 = -1;                 // q < 10: S[q]
        if (q >= 10) {                      // pair number q - 10 in the order (0,0) (0,1) .. (0,9) (1,1) ..
            int r = q - 10;
            k = 0;
            while (r >= 10 - k) {
                r -= 10 - k;
                ++k;
            }
            k2 = k + r;
        }
        // eight independent partial sums: the loop is a chain of LDS round trips + one dependent double add otherwise (3 waves per SIMD)
        const float *pa = sw + k, *pb = k2 < 0 ? nullptr : sw + k2;
        double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int t = slice;
        for (; t + 21 < nt; t += 24) {
            float va[8], vb[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                va[u] = pa[(t + 3 * u) * 5];
                vb[u] = pb ? pb[(t + 3 * u) * 5] : 1.0f;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc[u] += (double)va[u] * (double)vb[u];
        }
        for (; t < nt; t += 3) acc[0] += (double)pa[t * 5] * (pb ? (double)pb[t * 5] : 1.0);
        red[slice][q] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    __syncthreads();
    if (threadIdx.x < C0_NQ) part[((long)b * gridDim.x + blockIdx.x) * C0_NQ + threadIdx.x] = (red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x];
}
__global__ void w2v_gn_from_moments_len_kernel(const double *__restrict__ mom, const float *__restrict__ w, int C, const int *__restrict__ ns, float2 *__restrict__ stats, int BC) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= BC) return;
    const int b = i / C, c = i - b * C;
    const int L0 = w2v_l0(ns[b]);
    const double *m = mom + (long)b * C0_NQ;
    double wk[10];
#pragma unroll
    for (int k = 0; k < 10; ++k) wk[k] = (double)w[c * 10 + k];
    double s = 0.0, s2 = 0.0;
    int q = 10;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        s += wk[k] * m[k];
#pragma unroll
        for (int k2 = k; k2 < 10; ++k2, ++q) s2 += (k2 == k ? 1.0 : 2.0) * wk[k] * wk[k2] * m[q];
    }
    const double mean = s / L0;
    double var = s2 / L0 - mean * mean;
    if (var < 0) var = 0;
    stats[i] = float2{(float)mean, (float)(1.0 / sqrt(var + 1e-5))};
}
// the length variant: wav (B, N) padded rows, ns (B,) device table of the clips' own sample counts (10 <= ns[b] <= N); out (B, L0, C) with
// L0 = the rows of N samples; rows at or beyond a clip's own (ns[b] - 10) / 5 + 1 are written as zeros.  Same scratch as launch_w2v_conv0
hipError_t launch_w2v_conv0_lens(const float *wav, int B, int N, const int *ns, const float *w, const float *gamma, const float *beta,
                                 double2 *part, float2 *stats, float *out, int C, bool moments, hipStream_t s) {
    const int L0 = w2v_l0(N), ntb = (L0 + C0_TB - 1) / C0_TB;
    if (moments) {
        const int nblk = (L0 + C0_MB - 1) / C0_MB;
        double *pm = reinterpret_cast<double *>(part), *mom = pm + (size_t)B * nblk * C0_NQ;
        hipLaunchKernelGGL(w2v_conv0_moments_len_kernel, dim3(nblk, B), dim3(256), 0, s, wav, N, ns, pm);
        hipLaunchKernelGGL(w2v_moments_reduce_kernel, dim3((B * C0_NQ + 255) / 256), dim3(256), 0, s, pm, nblk, mom, B * C0_NQ);
        hipLaunchKernelGGL(w2v_gn_from_moments_len_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, mom, w, C, ns, stats, B * C);
    } else {
        hipLaunchKernelGGL(w2v_conv0_stats_len_kernel, dim3(ntb, B), dim3(256), 0, s, wav, N, ns, w, part, C);
        hipLaunchKernelGGL(w2v_gn_finalize_len_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, ntb, C, ns, stats, B * C);
    }
    hipLaunchKernelGGL(w2v_conv0_apply_len_kernel, dim3(ntb, B), dim3(256), 0, s, wav, N, L0, ns, w, stats, gamma, beta, out, C);
    return hipGetLastError();
}

// ---- row-wise LayerNorm: one wavefront per row, C = 64 * CPL -----------------------------------------------------
template <int CPL>
__device__ inline void ln_row(float (&v)[CPL], const float *gamma, const float *beta, int lane, float eps) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) s += v[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    const float mean = s * (1.0f / (64 * CPL));
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < CPL; ++i) { const float d = v[i] - mean; q = fmaf(d, d, q); }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) q += __shfl_xor(q, off);
    const float rstd = 1.0f / sqrtf(q * (1.0f / (64 * CPL)) + eps);
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = (v[i] - mean) * rstd * gamma[lane + 64 * i] + beta[lane + 64 * i];
}

template <int CPL>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float *__restrict__ x, int ldx, long M,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             const float *__restrict__ post_res, int ldr, int relu,
                                                             float *__restrict__ out, int ldo) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    float v[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = x[m * ldx + lane + 64 * i];
    ln_row<CPL>(v, gamma, beta, lane, 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        float y = v[i];
        if (post_res) y += post_res[m * ldr + lane + 64 * i];
        if (relu) y = y > 0.f ? y : 0.f;
        out[m * ldo + lane + 64 * i] = y;
    }
}

hipError_t launch_layernorm_rows(const float *x, int ldx, long M, int C, const float *gamma, const float *beta,
                                 const float *post_res, int ldr, int relu, float *out, int ldo, hipStream_t s) {
    dim3 grid((unsigned)((M + 3) / 4)), block(256);
    switch (C) {
        case 64: hipLaunchKernelGGL(layernorm_rows_kernel<1>, grid, block, 0, s, x, ldx, M, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 256: hipLaunchKernelGGL(layernorm_rows_kernel<4>, grid, block, 0, s, x, ldx, M, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 512: hipLaunchKernelGGL(layernorm_rows_kernel<8>, grid, block, 0, s, x, ldx, M, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 768: hipLaunchKernelGGL(layernorm_rows_kernel<12>, grid, block, 0, s, x, ldx, M, gamma, beta, post_res, ldr, relu, out, ldo); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the length variant (mixed passes): rows (b, t) of B clips padded to T rows; a row at or beyond its clip's lens[b] is written as zeros and its
// input is not read (one wavefront per row: the branch is wave-uniform).  The arithmetic of a valid row is ln_row's, as above
template <int CPL>
__global__ __launch_bounds__(256) void layernorm_rows_len_kernel(const float *__restrict__ x, int ldx, long M, int T, const int *__restrict__ lens,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 const float *__restrict__ post_res, int ldr, int relu,
                                                                 float *__restrict__ out, int ldo) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(m / T), t = (int)(m - (long)b * T);
    if (t >= lens[b]) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) out[m * ldo + lane + 64 * i] = 0.f;
        return;
    }
    float v[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = x[m * ldx + lane + 64 * i];
    ln_row<CPL>(v, gamma, beta, lane, 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) {
        float y = v[i];
        if (post_res) y += post_res[m * ldr + lane + 64 * i];
        if (relu) y = y > 0.f ? y : 0.f;
        out[m * ldo + lane + 64 * i] = y;
    }
}

hipError_t launch_layernorm_rows_lens(const float *x, int ldx, int B, int T, const int *lens, int C, const float *gamma, const float *beta,
                                      const float *post_res, int ldr, int relu, float *out, int ldo, hipStream_t s) {
    const long M = (long)B * T;
    dim3 grid((unsigned)((M + 3) / 4)), block(256);
    switch (C) {
        case 64: hipLaunchKernelGGL(layernorm_rows_len_kernel<1>, grid, block, 0, s, x, ldx, M, T, lens, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 256: hipLaunchKernelGGL(layernorm_rows_len_kernel<4>, grid, block, 0, s, x, ldx, M, T, lens, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 512: hipLaunchKernelGGL(layernorm_rows_len_kernel<8>, grid, block, 0, s, x, ldx, M, T, lens, gamma, beta, post_res, ldr, relu, out, ldo); break;
        case 768: hipLaunchKernelGGL(layernorm_rows_len_kernel<12>, grid, block, 0, s, x, ldx, M, T, lens, gamma, beta, post_res, ldr, relu, out, ldo); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- time interpolation (align_corners=False) + LayerNorm(512) --------------------------------------------------
// Source index of frame j: scale * (j + 0.5) - 0.5 as ONE fused multiply-add, the rounding of ATen's vectorized (AVX2 / AVX512) CPU
// kernels that made the reference's goldens (tests/test_face_oracle_golden.py::test_lerp_source_index_matches_aten); ATen's scalar
// kernel and the numpy oracle round the product first, which moves the lerp weight of a few frames by up to an ulp of the index.
__device__ inline float lerp_src_index(float scale, int j) {
    const float src = __builtin_fmaf(scale, (float)j + 0.5f, -0.5f);
    return src < 0.f ? 0.f : src;
}
__global__ __launch_bounds__(256) void lerp_ln_kernel(const float *__restrict__ x, int Lin, int T, long M,
                                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                                      float *__restrict__ out) {
    constexpr int CPL = 8, C = 512;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(m / T), j = (int)(m - (long)b * T);
    const float scale = (float)Lin / (float)T;
    const float src = lerp_src_index(scale, j);
    const int i0 = (int)floorf(src);
    const int i1 = min(i0 + 1, Lin - 1);
    const float l1 = src - (float)i0, l0 = 1.0f - l1;
    const float *r0 = x + ((long)b * Lin + i0) * C, *r1 = x + ((long)b * Lin + i1) * C;
    float v[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) v[i] = r0[lane + 64 * i] * l0 + r1[lane + 64 * i] * l1;
    ln_row<CPL>(v, gamma, beta, lane, 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) out[m * C + lane + 64 * i] = v[i];
}
hipError_t launch_lerp_ln(const float *x, int B, int Lin, int T, const float *gamma, const float *beta, float *out,
                          hipStream_t s) {
    const long M = (long)B * T;
    hipLaunchKernelGGL(lerp_ln_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, Lin, T, M, gamma, beta, out);
    return hipGetLastError();
}

// the length variant (mixed passes): x (B, Lin, 512) and out (B, T, 512) are padded; clip b interpolates ITS rows w2v_feature_rows(ns[b]) to ITS
// frames[b] frames with its own scale (the same expressions as above on the clip's own counts); frames at or beyond frames[b] are written as zeros
__global__ __launch_bounds__(256) void lerp_ln_len_kernel(const float *__restrict__ x, int Lin, int T, long M, const int *__restrict__ ns,
                                                          const int *__restrict__ frames, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float *__restrict__ out) {
    constexpr int CPL = 8, C = 512;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(m / T), j = (int)(m - (long)b * T);
    const int Tb = frames[b];
    if (j >= Tb) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) out[m * C + lane + 64 * i] = 0.f;
        return;
    }
    const int Lb = w2v_feature_rows(ns[b]);
    const float scale = (float)Lb / (float)Tb;
    const float src = lerp_src_index(scale, j);
    const int i0 = (int)floorf(src);
    const int i1 = min(i0 + 1, Lb - 1);
    const float l1 = src - (float)i0, l0 = 1.0f - l1;
    const float *r0 = x + ((long)b * Lin + i0) * C, *r1 = x + ((long)b * Lin + i1) * C;
    float v[CPL];
#pragma unroll
    // r0 l0 + r1 l1 as the uniform kernel's code has it: the product r1 l1 rounded, then ONE fused multiply-add.  Stated explicitly: left to
    // the compiler's contraction this kernel got packed math with the two products' roles swapped in every other channel (an ulp apart)
    for (int i = 0; i < CPL; ++i) v[i] = __builtin_fmaf(r0[lane + 64 * i], l0, r1[lane + 64 * i] * l1);
    ln_row<CPL>(v, gamma, beta, lane, 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) out[m * C + lane + 64 * i] = v[i];
}
hipError_t launch_lerp_ln_lens(const float *x, int B, int Lin, int T, const int *ns, const int *frames, const float *gamma, const float *beta,
                               float *out, hipStream_t s) {
    const long M = (long)B * T;
    hipLaunchKernelGGL(lerp_ln_len_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, Lin, T, M, ns, frames, gamma, beta, out);
    return hipGetLastError();
}

// ---- fused attention of one wav2vec2 encoder layer (HF eager_attention_forward: softmax(Q K^T * d^-0.5) V, wav2vec.py:76-143) ----
// One workgroup = 64 queries of one (clip, head); wave w owns queries 16 w .. 16 w + 15 and walks the keys in tiles of 64 that all
// four waves share through LDS (K and V as [key][d], rows pitched 68 floats).  Both products run on v_mfma_f32_16x16x4_f32 with the KEYS as the rows of the first product:
//     S^T[key][query] = K Q^T        lane (li, lg) ends up with keys 4 lg .. 4 lg + 3 of each 16-key block for query li
//     O^T[d][query]  += V^T P^T      ... which is exactly the B-operand fragment of the second product (k index = key 4 lg + e)
// so the probabilities never leave their registers, a query's running max / sum are two xor-shuffles across the four lane groups,
// and the (B, heads, T, T) score tensor of the launch-per-op form (QK^T GEMM -> softmax kernel -> V transpose kernel -> PV GEMM:
// 0.77 GB written and read back per layer at batch 64) does not exist.  Online soft-max over the key tiles (running max m, sum l,
// O rescaled by exp(m_old - m_new)): any T, no 2^31-entry score buffer.  fp32 throughout; the scale 2^-3 is exact.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int V> struct IC4 { static constexpr int value = V; };
constexpr int ATT_P = 68;
// all-reduce across the four 16-lane rows of a wave with the gfx950 row-swap instructions (VALU; a __shfl_xor is a ds_bpermute: an LDS
// round trip on the soft-max's critical path): v_permlane16_swap(x, x) -> {rows (0,0,2,2), rows (1,1,3,3)}, v_permlane32_swap(x, x) ->
// {lower half twice, upper half twice}
template <class Op> __device__ __forceinline__ float rows_allreduce(float x, Op op) {
    auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    x = op(__uint_as_float(a[0]), __uint_as_float(a[1]));
    auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
    return op(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__global__ __launch_bounds__(256, 2) void attention_kernel(const float *__restrict__ qkv, int T, int HID, int heads, int nz, float scale,
                                                           float *__restrict__ out) {
    __shared__ float Ks[64 * ATT_P];
    __shared__ float Vs[64 * ATT_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    // workgroup id -> (clip-head z, query tile): consecutive ids go to consecutive XCDs, so the nq query tiles of one (clip, head)
    // take ids that are congruent mod 8 — they run on ONE XCD, back to back, and find K / V of their (clip, head) in its L2
    // (with the query tile as the fastest grid index every tile of a (clip, head) pulled its own copy over the fabric:
    // 708 MB per launch at batch 64 against 236 MB of compulsory traffic)
    const int nq = (T + 63) >> 6;
    const int xcd = blockIdx.x & 7, grp = blockIdx.x >> 3;
    const int z = (grp / nq) * 8 + xcd;
    if (z >= nz) return;
    const int b = z / heads, h = z - b * heads;
    const int q0 = (grp % nq) * 64 + wave * 16;
    const long ld = 3L * HID;
    const int Tp = T;   // clip stride in rows (attention_tile.inc)
    const float *base = qkv + (long)b * Tp * ld + h * 64;
#include "attention_tile.inc"
}
// Mixed passes: clips of different lengths padded to Tp rows; clip b has frames[b] keys and queries in rows [b Tp, b Tp + frames[b]) of qkv and
// out.  work[workgroup id] = (clip * heads + head) << 10 | query tile, or -1 for an id without a tile (face.cpp::face_mixed_grid: the tiles of
// one (clip, head) carry ids of equal residue mod 8, as above; query tiles wholly beyond frames[b] are not in the list).  The key-tile walk, the
// ragged last tile and the online soft-max of a clip are those of the clip alone; K / V rows at or beyond frames[b] are never read, out rows
// there are not written.
__global__ __launch_bounds__(256, 2) void attention_mixed_kernel(const float *__restrict__ qkv, int Tp, int HID, int heads,
                                                                 const int *__restrict__ work, const int *__restrict__ frames, float scale,
                                                                 float *__restrict__ out) {
    __shared__ float Ks[64 * ATT_P];
    __shared__ float Vs[64 * ATT_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int e = work[blockIdx.x];
    if (e < 0) return;
    const int z = e >> 10, b = z / heads, h = z - b * heads;
    const int T = frames[b];
    const int q0 = (e & 1023) * 64 + wave * 16;
    const long ld = 3L * HID;
    const float *base = qkv + (long)b * Tp * ld + h * 64;
#include "attention_tile.inc"
}
// qkv (B, T, 3 HID) rows [q | k | v], heads of 64 channels -> out (B, T, HID) = concatenated heads' softmax(q k^T * scale) v
hipError_t launch_attention(const float *qkv, int B, int T, int HID, int heads, float scale, float *out, hipStream_t s) {
    if (HID != heads * 64 || B < 1 || T < 1 || (long)B * heads * ((T + 63) / 64) > (1l << 30)) return hipErrorInvalidValue;
    const int nq = (T + 63) / 64, nz = B * heads;
    hipLaunchKernelGGL(attention_kernel, dim3((unsigned)(((nz + 7) / 8) * 8 * nq)), dim3(256), 0, s, qkv, T, HID, heads, nz, scale, out);
    return hipGetLastError();
}
// the mixed form: qkv (B, Tp, 3 HID), out (B, Tp, HID); `work` = n_work device entries as attention_mixed_kernel reads them, frames (B,) device
hipError_t launch_attention_mixed(const float *qkv, int Tp, int HID, int heads, const int *work, int n_work, const int *frames, float scale,
                                  float *out, hipStream_t s) {
    if (HID != heads * 64 || Tp < 1 || Tp > 65536 || n_work < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_mixed_kernel, dim3((unsigned)n_work), dim3(256), 0, s, qkv, Tp, HID, heads, work, frames, scale, out);
    return hipGetLastError();
}

// dst[0 .. n) = the words of `w`, carried by the launch's own arguments: a host table reaches a stream's buffer in stream order, without a
// host buffer that has to outlive the call and without a copy that waits for the stream
__global__ void put_words_kernel(int *__restrict__ dst, const PutWords w, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = w.v[i];
}
hipError_t launch_put_words(int *dst, const int *host, long n, hipStream_t s) {
    PutWords w;
    for (long i0 = 0; i0 < n; i0 += PutWords::N) {
        const int c = (int)(n - i0 < PutWords::N ? n - i0 : PutWords::N);
        std::memcpy(w.v, host + i0, (size_t)c * sizeof(int));
        hipLaunchKernelGGL(put_words_kernel, dim3((c + 255) / 256), dim3(256), 0, s, dst + i0, w, c);
    }
    return hipGetLastError();
}

// ---- id channels: x[b][t][col0 + j] = bias[j] + sum_c W[j][c] * id[b][c] ----------------------------------------
__global__ void fill_id_kernel(const float *__restrict__ id, int nc, const float *__restrict__ w, const float *__restrict__ bias,
                               int nj, float *__restrict__ x, int ld, int col0, long rows, int T) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nj) return;
    const long m = i / nj;
    const int j = (int)(i - m * nj);
    const int b = (int)(m / T);
    float v = bias[j];
    for (int c = 0; c < nc; ++c) v = fmaf(w[j * nc + c], id[b * nc + c], v);
    x[m * ld + col0 + j] = v;
}
hipError_t launch_fill_id(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0,
                          int B, int T, hipStream_t s) {
    const long n = (long)B * T * nj;
    hipLaunchKernelGGL(fill_id_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, id, nc, w, bias, nj, x, ld, col0,
                       (long)B * T, T);
    return hipGetLastError();
}

// the length variant (mixed passes): B clips padded to T rows; rows at or beyond lens[b] get zeros in the id columns
__global__ void fill_id_len_kernel(const float *__restrict__ id, int nc, const float *__restrict__ w, const float *__restrict__ bias,
                                   int nj, float *__restrict__ x, int ld, int col0, long rows, int T, const int *__restrict__ lens) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * nj) return;
    const long m = i / nj;
    const int j = (int)(i - m * nj);
    const int b = (int)(m / T);
    float v = 0.f;
    if ((int)(m - (long)b * T) < lens[b]) {
        v = bias[j];
        for (int c = 0; c < nc; ++c) v = fmaf(w[j * nc + c], id[b * nc + c], v);
    }
    x[m * ld + col0 + j] = v;
}
hipError_t launch_fill_id_lens(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0,
                               int B, int T, const int *lens, hipStream_t s) {
    const long n = (long)B * T * nj;
    hipLaunchKernelGGL(fill_id_len_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, id, nc, w, bias, nj, x, ld, col0,
                       (long)B * T, T, lens);
    return hipGetLastError();
}

// ---- packed mixed passes (kernels.h, "packed mixed passes"; face.cpp::face_packed_layout): the clips' own rows back to back.  Kernels of their
// own: the uniform kernels and the length variants keep their names and their code ----
// the clip that owns row g of a packed axis: the last b with off[b] <= g (off ascending, off[0] = 0, every clip owns at least one row)
__device__ __forceinline__ int packed_clip(const int *__restrict__ off, int B, int g) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
constexpr int C0_PB = 64;   // rows per block of the packed apply kernel: a clip's segment is a whole number of them
// w2v_conv0_apply_len_kernel's statements on one block of 64 rows of the packed axis: rows [off[b], off[b] + L0(ns[b])) are clip b's, the rest of
// its segment is zeros (what a neighbour's seam rows read; no valid row reads them)
__global__ __launch_bounds__(256) void w2v_conv0_apply_packed_kernel(const float *__restrict__ wav, int N, int B, const int *__restrict__ ns,
                                                                 const int *__restrict__ off, const float *__restrict__ w,
                                                                 const float2 *__restrict__ stats, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float *__restrict__ out, int C) {
    __shared__ float sw[C0_PB * 5 + 16];
    const int g0 = blockIdx.x * C0_PB;
    const int b = packed_clip(off, B, g0), t0 = g0 - off[b];
    const int n = ns[b];
    const int nt = min(C0_PB, w2v_l0(n) - t0);   // >= 1: the segment ends within 64 rows of the clip's last
    for (int i = threadIdx.x; i < nt * 5 + 5; i += 256) {
        const int idx = t0 * 5 + i;
        sw[i] = idx < n ? wav[(long)b * N + idx] : 0.f;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float wk[10];
#pragma unroll
        for (int k = 0; k < 10; ++k) wk[k] = w[c * 10 + k];
        const float2 st = stats[b * C + c];
        const float g = gamma[c], be = beta[c];
        for (int t = 0; t < nt; ++t) {
            float v = 0.f;
#pragma unroll
            for (int k = 0; k < 10; ++k) v = fmaf(wk[k], sw[t * 5 + k], v);
            v = (v - st.x) * st.y * g + be;
            out[((long)g0 + t) * C + c] = gelu_erf(v);
        }
        for (int t = nt; t < C0_PB; ++t) out[((long)g0 + t) * C + c] = 0.f;
    }
}
hipError_t launch_w2v_conv0_packed(const float *wav, int B, int N, const int *ns, const int *off, int feat_rows, const float *w,
                                   const float *gamma, const float *beta, double2 *part, float2 *stats, float *out, int C, bool moments,
                                   hipStream_t s) {
    if (feat_rows < C0_PB || feat_rows % C0_PB) return hipErrorInvalidValue;
    const int L0 = w2v_l0(N), ntb = (L0 + C0_TB - 1) / C0_TB;
    if (moments) {
        const int nblk = (L0 + C0_MB - 1) / C0_MB;
        double *pm = reinterpret_cast<double *>(part), *mom = pm + (size_t)B * nblk * C0_NQ;
        hipLaunchKernelGGL(w2v_conv0_moments_len_kernel, dim3(nblk, B), dim3(256), 0, s, wav, N, ns, pm);
        hipLaunchKernelGGL(w2v_moments_reduce_kernel, dim3((B * C0_NQ + 255) / 256), dim3(256), 0, s, pm, nblk, mom, B * C0_NQ);
        hipLaunchKernelGGL(w2v_gn_from_moments_len_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, mom, w, C, ns, stats, B * C);
    } else {
        hipLaunchKernelGGL(w2v_conv0_stats_len_kernel, dim3(ntb, B), dim3(256), 0, s, wav, N, ns, w, part, C);
        hipLaunchKernelGGL(w2v_gn_finalize_len_kernel, dim3((B * C + 255) / 256), dim3(256), 0, s, part, ntb, C, ns, stats, B * C);
    }
    hipLaunchKernelGGL(w2v_conv0_apply_packed_kernel, dim3(feat_rows / C0_PB), dim3(256), 0, s, wav, N, B, ns, off, w, stats, gamma, beta, out, C);
    return hipGetLastError();
}

// lerp_ln_len_kernel reading clip b's level-6 rows at off[b] >> 6 of the packed axis; out (B, T, 512) padded, the same values and zeros
__global__ __launch_bounds__(256) void lerp_ln_packed_kernel(const float *__restrict__ x, int T, long M, const int *__restrict__ ns,
                                                             const int *__restrict__ frames, const int *__restrict__ off,
                                                             const float *__restrict__ gamma, const float *__restrict__ beta,
                                                             float *__restrict__ out) {
    constexpr int CPL = 8, C = 512;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(m / T), j = (int)(m - (long)b * T);
    const int Tb = frames[b];
    if (j >= Tb) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) out[m * C + lane + 64 * i] = 0.f;
        return;
    }
    const int Lb = w2v_feature_rows(ns[b]);
    const float scale = (float)Lb / (float)Tb;
    const float src = lerp_src_index(scale, j);
    const int i0 = (int)floorf(src);
    const int i1 = min(i0 + 1, Lb - 1);
    const float l1 = src - (float)i0, l0 = 1.0f - l1;
    const long first = off[b] >> 6;
    const float *r0 = x + (first + i0) * C, *r1 = x + (first + i1) * C;
    float v[CPL];
#pragma unroll
    // the product r1 l1 rounded, then ONE fused multiply-add: the order lerp_ln_kernel's code has and lerp_ln_len_kernel states
    for (int i = 0; i < CPL; ++i) v[i] = __builtin_fmaf(r0[lane + 64 * i], l0, r1[lane + 64 * i] * l1);
    ln_row<CPL>(v, gamma, beta, lane, 1e-5f);
#pragma unroll
    for (int i = 0; i < CPL; ++i) out[m * C + lane + 64 * i] = v[i];
}
hipError_t launch_lerp_ln_packed(const float *x, int B, int T, const int *ns, const int *frames, const int *off, const float *gamma,
                                 const float *beta, float *out, hipStream_t s) {
    const long M = (long)B * T;
    hipLaunchKernelGGL(lerp_ln_packed_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, x, T, M, ns, frames, off, gamma, beta, out);
    return hipGetLastError();
}

// one wavefront per row, float4 per lane
__global__ __launch_bounds__(256) void pack_rows_kernel(const float *__restrict__ src, int T, int C4, const int *__restrict__ row0, int B,
                                                        int rows, float *__restrict__ dst) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int lane = threadIdx.x & 63;
    const int b = packed_clip(row0, B, m), t = m - row0[b];
    const float4 *sp = reinterpret_cast<const float4 *>(src) + ((long)b * T + t) * C4;
    float4 *dp = reinterpret_cast<float4 *>(dst) + (long)m * C4;
    for (int i = lane; i < C4; i += 64) dp[i] = sp[i];
}
__global__ __launch_bounds__(256) void unpack_rows_kernel(const float *__restrict__ src, const int *__restrict__ row0,
                                                          const int *__restrict__ frames, int T, int C4, long M, float *__restrict__ dst) {
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const int lane = threadIdx.x & 63;
    const int b = (int)(m / T), t = (int)(m - (long)b * T);
    float4 *dp = reinterpret_cast<float4 *>(dst) + m * C4;
    if (t >= frames[b]) {
        for (int i = lane; i < C4; i += 64) dp[i] = float4{0.f, 0.f, 0.f, 0.f};
        return;
    }
    const float4 *sp = reinterpret_cast<const float4 *>(src) + ((long)row0[b] + t) * C4;
    for (int i = lane; i < C4; i += 64) dp[i] = sp[i];
}
hipError_t launch_pack_rows(const float *src, int B, int T, int C, const int *row0, int rows, float *dst, hipStream_t s) {
    if (B < 1 || T < 1 || rows < 1 || C < 4 || C % 4) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, src, T, C / 4, row0, B, rows, dst);
    return hipGetLastError();
}
hipError_t launch_unpack_rows(const float *src, const int *row0, const int *frames, int B, int T, int C, float *dst, hipStream_t s) {
    if (B < 1 || T < 1 || C < 4 || C % 4) return hipErrorInvalidValue;
    const long M = (long)B * T;
    hipLaunchKernelGGL(unpack_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, src, row0, frames, T, C / 4, M, dst);
    return hipGetLastError();
}

// attention_mixed_kernel on packed rows: clip b's keys and queries are rows [row0[b], row0[b] + frames[b]) of qkv and out.  Same work list, same
// tile body (attention_tile.inc, a third compilation: its clip stride is 0 here, the clip's first row is folded into both pointers)
__global__ __launch_bounds__(256, 2) void attention_packed_kernel(const float *__restrict__ qkv, int HID, int heads,
                                                                  const int *__restrict__ work, const int *__restrict__ frames,
                                                                  const int *__restrict__ row0, float scale, float *__restrict__ out_rows) {
    __shared__ float Ks[64 * ATT_P];
    __shared__ float Vs[64 * ATT_P];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
    const int e = work[blockIdx.x];
    if (e < 0) return;
    const int z = e >> 10, b = z / heads, h = z - b * heads;
    const int T = frames[b];
    const int q0 = (e & 1023) * 64 + wave * 16;
    const long ld = 3L * HID, first = row0[b];
    constexpr int Tp = 0;
    const float *base = qkv + first * ld + h * 64;
    float *__restrict__ out = out_rows + first * HID;
#include "attention_tile.inc"
}
hipError_t launch_attention_packed(const float *qkv, int HID, int heads, const int *work, int n_work, const int *frames, const int *row0,
                                   float scale, float *out, hipStream_t s) {
    if (HID != heads * 64 || n_work < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attention_packed_kernel, dim3((unsigned)n_work), dim3(256), 0, s, qkv, HID, heads, work, frames, row0, scale, out);
    return hipGetLastError();
}

}  // namespace ts
