// Device audio front-end kernels (the GEMM-shaped parts — the mel projection, the DCT — run on conv_gemm_f32):
//   resample_polyphase   torchaudio.transforms.Resample (sinc_interp_hann) as a polyphase FIR
//   stft_power           reflect padding (center=True) + framing (n_fft 2048, hop) + periodic Hann window + real FFT + |X|^2, one frame
//                        per workgroup, zero-padded to a multiple of 32 bins
//   db_topdb             10*log10(clamp(x, 1e-10)) and the per-clip clamp at (max - top_db)
// Reference call site: data_utils/utils.py:148-231 (get_mfcc_ta) -> torchaudio.transforms.{Resample, MFCC}.
// Every kernel family comes in up to three forms: uniform (B clips of one length), `_len` (mixed passes: clips of different lengths padded to
// one width) and `_stream` (wav sessions: rows indexed by absolute sample index).  A recording gives the same bits in all of them because each
// family has ONE __device__ body; a form's __global__ shell only decodes its row, says how a sample is fetched and writes its zero fill.
#include "kernels.h"

namespace ts {

// Samples [lo, hi) of a recording, sample i at xb[i - lo]; a tap outside is a zero.  Clips: lo = 0, hi = N (uniform) or the clip's own count
// (_len), I = int.  Wav sessions (_stream): [x0, n) by absolute index, I = long; i >= x0 covers i >= 0: x0 is never negative
template <class I>
struct Taps {
    const float *xb;
    I lo, hi;
};
// output j = sum_k kern[j % nnew][k] * xpad[(j / nnew) * norig + k],  xpad = the recording shifted by `width` zeros on the left
template <class I>
__device__ __forceinline__ float polyphase_sum(Taps<I> taps, I j, const float *kern, int norig, int nnew, int width, int kw) {
    const I wdw = j / nnew;
    const int ph = (int)(j - wdw * nnew);
    const float *kr = kern + ph * kw;
    const I base = wdw * norig - width;
    float acc = 0.f;
    for (int k = 0; k < kw; ++k) {
        const I i = base + k;
        if (i >= taps.lo && i < taps.hi) acc = fmaf(kr[k], taps.xb[i - taps.lo], acc);
    }
    return acc;
}
// The same sum with the polyphase table and the block's input window staged in LDS (the plain kernel fetches 2 kw values per output
// through L1: 58 % of the front-end once the STFT became an FFT).  Same terms in the same order — taps that fall outside the clip
// multiply a staged zero instead of being skipped, which leaves the fma chain's value unchanged — so the samples are bit-identical.
// Two halves, so that a shell can leave between them: polyphase_stage is for every thread of the block that starts at output j0 and ends in
// the barrier; polyphase_staged_sum is output j of that block.
template <class I>
__device__ __forceinline__ void polyphase_stage(Taps<I> taps, I j0, const float *kern, int norig, int nnew, int width, int kw, int nwin) {
    extern __shared__ float sm[];
    float *sk = sm, *sw = sm + nnew * kw;
    const I base = (j0 / nnew) * norig - width;              // first input sample any output of this block touches
    for (int i = threadIdx.x; i < nnew * kw; i += 256) sk[i] = kern[i];
    for (int i = threadIdx.x; i < nwin; i += 256) {
        const I g = base + i;
        sw[i] = (g >= taps.lo && g < taps.hi) ? taps.xb[g - taps.lo] : 0.f;
    }
    __syncthreads();
}
template <class I>
__device__ __forceinline__ float polyphase_staged_sum(I j0, I j, int norig, int nnew, int width, int kw) {
    extern __shared__ float sm[];
    const float *sk = sm, *sw = sm + nnew * kw;
    const I base = (j0 / nnew) * norig - width;
    const I wdw = j / nnew;
    const int ph = (int)(j - wdw * nnew);
    const float *kr = sk + ph * kw, *xw = sw + (wdw * norig - width - base);
    float acc = 0.f;
    for (int k = 0; k < kw; ++k) acc = fmaf(kr[k], xw[k], acc);
    return acc;
}
// the staged form's input window of 256 consecutive outputs (wherever they start), its LDS bytes, and whether it is taken: by the rate ratio
// alone — small ratios (16 k -> 22 k: 11 x 22 taps) stage, big ones (44.1 k -> 22 k: 220 x 467) keep the plain kernel — so every form of a
// handle takes the same one
struct PolyphaseLds {
    int nwin;
    size_t bytes;
    bool staged;
};
static PolyphaseLds polyphase_lds(int norig, int nnew, int kw) {
    const int nwin = (255 / nnew + 1) * norig + kw;
    const size_t bytes = ((size_t)nnew * kw + nwin) * sizeof(float);
    return {nwin, bytes, bytes <= 48 * 1024};
}

__global__ void resample_polyphase_kernel(const float *__restrict__ x, int N, const float *__restrict__ kern, int norig,
                                          int nnew, int width, int kw, float *__restrict__ out, int Nout) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Nout) return;
    out[(long)b * Nout + j] = polyphase_sum(Taps<int>{x + (long)b * N, 0, N}, j, kern, norig, nnew, width, kw);
}
__global__ __launch_bounds__(256) void resample_polyphase_lds_kernel(const float *__restrict__ x, int N, const float *__restrict__ kern,
                                                                     int norig, int nnew, int width, int kw, float *__restrict__ out,
                                                                     int Nout, int nwin) {
    const int b = blockIdx.y, j0 = blockIdx.x * 256;
    polyphase_stage(Taps<int>{x + (long)b * N, 0, N}, j0, kern, norig, nnew, width, kw, nwin);
    const int j = j0 + threadIdx.x;
    if (j >= Nout) return;
    out[(long)b * Nout + j] = polyphase_staged_sum(j0, j, norig, nnew, width, kw);
}
hipError_t launch_resample_polyphase(const float *x, int B, int N, const float *kern, int norig, int nnew, int width, int kw,
                                     float *out, int Nout, hipStream_t s) {
    const PolyphaseLds l = polyphase_lds(norig, nnew, kw);
    if (l.staged) {
        hipLaunchKernelGGL(resample_polyphase_lds_kernel, dim3((Nout + 255) / 256, B), dim3(256), l.bytes, s, x, N, kern, norig, nnew, width,
                           kw, out, Nout, l.nwin);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(resample_polyphase_kernel, dim3((Nout + 255) / 256, B), dim3(256), 0, s, x, N, kern, norig, nnew, width,
                       kw, out, Nout);
    return hipGetLastError();
}

// Band-limited interpolation with a table-driven Kaiser-windowed sinc (J. O. Smith's algorithm as published in resampy,
// the resampler behind librosa.load(sr=...) in the reference's pinned librosa 0.9.2: data_utils/utils.py:194).
// win[0..nwin) is the right half of the filter sampled `num_table` times per zero crossing, delta[i] = win[i+1]-win[i].
// Output sample t sits at input time t / ratio; left wing walks x[n], x[n-1], ..., right wing x[n+1], x[n+2], ...
// One thread per output sample; the two table taps of a weight are adjacent floats.  xb: the recording's own N samples.
__device__ __forceinline__ float kaiser_sample(const float *__restrict__ xb, int N, int t, const float *__restrict__ win,
                                               const float *__restrict__ delta, int nwin, int num_table, double ratio) {
    const double scale = ratio < 1.0 ? ratio : 1.0;
    const int index_step = (int)(scale * num_table);
    const double time_register = (double)t / ratio;
    const int n = (int)time_register;
    double frac = scale * (time_register - n);
    double index_frac = frac * num_table;
    int offset = (int)index_frac;
    double eta = index_frac - offset;
    int i_max = (nwin - offset) / index_step;
    i_max = i_max < n + 1 ? i_max : n + 1;
    double acc = 0.0;
    for (int i = 0; i < i_max; ++i) {
        const int k = offset + i * index_step;
        acc += ((double)win[k] + eta * (double)delta[k]) * (double)xb[n - i];
    }
    frac = scale - frac;
    index_frac = frac * num_table;
    offset = (int)index_frac;
    eta = index_frac - offset;
    int k_max = (nwin - offset) / index_step;
    k_max = k_max < N - n - 1 ? k_max : N - n - 1;
    for (int k2 = 0; k2 < k_max; ++k2) {
        const int k = offset + k2 * index_step;
        acc += ((double)win[k] + eta * (double)delta[k]) * (double)xb[n + k2 + 1];
    }
    return (float)(acc * scale);   // resampy scales the filter by the ratio when decimating (unit DC gain)
}
__global__ void resample_kaiser_kernel(const float *__restrict__ x, int N, const float *__restrict__ win,
                                       const float *__restrict__ delta, int nwin, int num_table, double ratio,
                                       float *__restrict__ out, int Nout, int ldo) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Nout) return;
    out[(long)b * ldo + t] = kaiser_sample(x + (long)b * N, N, t, win, delta, nwin, num_table, ratio);
}
hipError_t launch_resample_kaiser(const float *x, int B, int N, const float *win, const float *delta, int nwin, int num_table,
                                  double ratio, float *out, int Nout, int ldo, hipStream_t s) {
    hipLaunchKernelGGL(resample_kaiser_kernel, dim3((Nout + 255) / 256, B), dim3(256), 0, s, x, N, win, delta, nwin, num_table,
                       ratio, out, Nout, ldo);
    return hipGetLastError();
}

// STFT power spectrum of one frame per workgroup: reflect padding (center=True) + framing + periodic Hann window + a 2048-point real
// FFT + |X|^2, fused (rounds 1-3 ran the transform as a 2048 x 2050 DFT matrix on conv_gemm_f32: 1.26 GMAC per 10 s clip, 150 x the
// arithmetic of an FFT and the largest item of the front-end).  The real transform is a 1024-point complex FFT of z[n] = x[2n] + i x[2n+1]
// — five radix-4 Stockham passes (auto-sorting, no bit reversal) through two LDS buffers, one butterfly per thread per pass, twiddles from
// a table computed in double — followed by the even / odd split X[k] = E[k] - i w^k O[k].  Rounding error grows with log2 N instead of
// sqrt N: closer to the float64 twin than the DFT matrix was.  pw[(b T + t)][0 .. ldp): bins 0 .. 1024, then zeros.
typedef float f32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f32x2 cmul(f32x2 a, f32x2 b) { return f32x2{a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]}; }
// sample(n) = windowed sample n of the frame (frame_window of rounds 1-3), n < 2048: the one thing the forms differ in.  out: the frame's row
template <class Sample>
__device__ __forceinline__ void stft_frame_power(Sample sample, const f32x2 *__restrict__ tw1024, const f32x2 *__restrict__ tw2048,
                                                 float *__restrict__ out, int ldp) {
    __shared__ f32x2 bufA[1024], bufB[1024];
    const int j = threadIdx.x;
    auto butterfly = [](f32x2 &v0, f32x2 &v1, f32x2 &v2, f32x2 &v3) {   // 4-point DFT, outputs in natural order
        const f32x2 a = v0 + v2, bb = v0 - v2, c = v1 + v3, d0 = v1 - v3;
        const f32x2 d = {d0[1], -d0[0]};                                  // (v1 - v3) * (-i)
        v0 = a + c; v2 = a - c; v1 = bb + d; v3 = bb - d;
    };
    f32x2 v[4];
    // pass 0 (Ns = 1): inputs straight from the waveform, no twiddles
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int n = j + 256 * r;
        v[r] = f32x2{sample(2 * n), sample(2 * n + 1)};
    }
    butterfly(v[0], v[1], v[2], v[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) bufA[j * 4 + r] = v[r];
    __syncthreads();
    // passes 1..4: Ns = 4, 16, 64, 256; twiddle of input r = exp(-2 pi i r (j mod Ns) / (4 Ns)) = tw1024[r (j mod Ns) (256 / Ns)]
    f32x2 *src = bufA, *dst = bufB;
#pragma unroll
    for (int p = 1; p < 5; ++p) {
        const int Ns = 1 << (2 * p), k = j & (Ns - 1), step = 256 >> (2 * p);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            v[r] = src[j + 256 * r];
            if (r) v[r] = cmul(v[r], tw1024[r * k * step]);
        }
        butterfly(v[0], v[1], v[2], v[3]);
        const int base = ((j - k) << 2) + k;
#pragma unroll
        for (int r = 0; r < 4; ++r) dst[base + r * Ns] = v[r];
        __syncthreads();
        f32x2 *tmp = src; src = dst; dst = tmp;
    }
    // src = Z in natural order.  X[k] = E - i w^k O, E = (Z[k] + conj Z[1024 - k]) / 2, O = (Z[k] - conj Z[1024 - k]) / 2, w = exp(-2 pi i / 2048)
    for (int k = j; k < ldp; k += 256) {
        float val = 0.f;
        if (k <= 1024) {
            const f32x2 zk = src[k & 1023], zn0 = src[(1024 - k) & 1023];
            const f32x2 zn = {zn0[0], -zn0[1]};
            const f32x2 e = (zk + zn) * 0.5f, o = (zk - zn) * 0.5f;
            const f32x2 tt = cmul(tw2048[k], o);
            const float xr = e[0] + tt[1], xi = e[1] - tt[0];
            val = xr * xr + xi * xi;
        }
        out[k] = val;
    }
}
__global__ __launch_bounds__(256) void stft_power_kernel(const float *__restrict__ x, int N, int T, int hop, const float *__restrict__ win,
                                                         const f32x2 *__restrict__ tw1024, const f32x2 *__restrict__ tw2048,
                                                         float *__restrict__ pw, int ldp) {
    const long row = blockIdx.x;   // b * T + t
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const float *xb = x + (long)b * N;
    auto sample = [&](int n) {
        int i = t * hop + n - 1024;
        if (i < 0) i = -i;
        if (i >= N) i = 2 * (N - 1) - i;
        i = i < 0 ? 0 : (i >= N ? N - 1 : i);
        return xb[i] * win[n];
    };
    stft_frame_power(sample, tw1024, tw2048, pw + row * ldp, ldp);
}
hipError_t launch_stft_power(const float *x, int B, int N, int T, int hop, const float *win, const float *tw1024, const float *tw2048,
                             float *pw, int ldp, hipStream_t s) {
    hipLaunchKernelGGL(stft_power_kernel, dim3((unsigned)((long)B * T)), dim3(256), 0, s, x, N, T, hop, win,
                       reinterpret_cast<const f32x2 *>(tw1024), reinterpret_cast<const f32x2 *>(tw2048), pw, ldp);
    return hipGetLastError();
}

// The decibel expression of every dB kernel, and the maximum of mx over the 256 threads of a workgroup (sm: 4 floats of LDS; one barrier)
__device__ __forceinline__ float db_of(float x) { return 10.0f * log10f(fmaxf(x, 1e-10f)); }
__device__ __forceinline__ float block_max_256(float mx, float (&sm)[4]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = mx;
    __syncthreads();
    return fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
}

// one workgroup per clip: x_db = 10 log10(max(x, 1e-10)); clamp at (clip max - top_db); in place
__global__ __launch_bounds__(256) void db_topdb_kernel(float *__restrict__ mel, long per_clip, float top_db) {
    __shared__ float sm[4];
    float *p = mel + (long)blockIdx.x * per_clip;
    float mx = -INFINITY;
    for (long i = threadIdx.x; i < per_clip; i += 256) {
        const float v = db_of(p[i]);
        p[i] = v;
        mx = fmaxf(mx, v);
    }
    const float lo = block_max_256(mx, sm) - top_db;
    for (long i = threadIdx.x; i < per_clip; i += 256) p[i] = fmaxf(p[i], lo);
}
hipError_t launch_db_topdb(float *mel, int B, long per_clip, float top_db, hipStream_t s) {
    hipLaunchKernelGGL(db_topdb_kernel, dim3(B), dim3(256), 0, s, mel, per_clip, top_db);
    return hipGetLastError();
}

// ---- length variants (mixed front-end passes: B recordings of different lengths, padded to N samples each; `ns` is the DEVICE table of the
// recordings' own sample counts at the input rate).  Each hands the shared body, from ns[b], what the uniform kernel hands it from N, Nout
// and T — the resampled length ceil(ns[b] nnew / norig), the frame count of that length — so a valid element is the uniform kernel's on the
// recording alone; everything beyond a recording's own length is written as 0, and samples at or beyond ns[b] are never read. ----
// (a count outside [0, N] is an error of the caller that the entries refuse from the host table; clamped, a device table that disagrees with
// it still cannot take a kernel outside its buffers)
__device__ __forceinline__ int clamp_count(int n, int N) { return n < 0 ? 0 : (n > N ? N : n); }
__device__ __forceinline__ int resampled_len_of(int n, int norig, int nnew) { return (int)(((long)nnew * n + norig - 1) / norig); }

__global__ void resample_polyphase_len_kernel(const float *__restrict__ x, int N, const int *__restrict__ ns, const float *__restrict__ kern,
                                              int norig, int nnew, int width, int kw, float *__restrict__ out, int Nout) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= Nout) return;
    const int Nb = clamp_count(ns[b], N);
    if (j >= resampled_len_of(Nb, norig, nnew)) {
        out[(long)b * Nout + j] = 0.f;
        return;
    }
    out[(long)b * Nout + j] = polyphase_sum(Taps<int>{x + (long)b * N, 0, Nb}, j, kern, norig, nnew, width, kw);
}
__global__ __launch_bounds__(256) void resample_polyphase_lds_len_kernel(const float *__restrict__ x, int N, const int *__restrict__ ns,
                                                                         const float *__restrict__ kern, int norig, int nnew, int width,
                                                                         int kw, float *__restrict__ out, int Nout, int nwin) {
    const int b = blockIdx.y, j0 = blockIdx.x * 256;
    const int Nb = clamp_count(ns[b], N), Nout_b = resampled_len_of(Nb, norig, nnew);
    const int j = j0 + threadIdx.x;
    if (j0 >= Nout_b) {                                       // a block wholly beyond the recording: its zeros, nothing staged
        if (j < Nout) out[(long)b * Nout + j] = 0.f;
        return;
    }
    polyphase_stage(Taps<int>{x + (long)b * N, 0, Nb}, j0, kern, norig, nnew, width, kw, nwin);
    if (j >= Nout) return;
    if (j >= Nout_b) {
        out[(long)b * Nout + j] = 0.f;
        return;
    }
    out[(long)b * Nout + j] = polyphase_staged_sum(j0, j, norig, nnew, width, kw);
}
// rows of N samples in, rows of Nout = ceil(N nnew / norig) samples out
hipError_t launch_resample_polyphase_lens(const float *x, int B, int N, const int *ns, const float *kern, int norig, int nnew, int width,
                                          int kw, float *out, int Nout, hipStream_t s) {
    const PolyphaseLds l = polyphase_lds(norig, nnew, kw);
    if (l.staged) {
        hipLaunchKernelGGL(resample_polyphase_lds_len_kernel, dim3((Nout + 255) / 256, B), dim3(256), l.bytes, s, x, N, ns, kern, norig, nnew,
                           width, kw, out, Nout, l.nwin);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(resample_polyphase_len_kernel, dim3((Nout + 255) / 256, B), dim3(256), 0, s, x, N, ns, kern, norig, nnew, width,
                       kw, out, Nout);
    return hipGetLastError();
}

// out[b][j] = x[b][j] for j < ns[b], 0 up to the row width (a mixed pass at equal rates: the copy of the uniform entries with its padding)
__global__ void copy_samples_len_kernel(const float *__restrict__ x, int N, const int *__restrict__ ns, float *__restrict__ out) {
    const int b = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= N) return;
    out[(long)b * N + j] = j < clamp_count(ns[b], N) ? x[(long)b * N + j] : 0.f;
}
hipError_t launch_copy_samples_lens(const float *x, int B, int N, const int *ns, float *out, hipStream_t s) {
    hipLaunchKernelGGL(copy_samples_len_kernel, dim3((N + 255) / 256, B), dim3(256), 0, s, x, N, ns, out);
    return hipGetLastError();
}

// rows of N samples in; row b holds ns[b]: int(ns[b] ratio) samples computed, zeros from there to the row width ldo (fix_length's one
// sample and the padding)
__global__ void resample_kaiser_len_kernel(const float *__restrict__ x, int N, const int *__restrict__ ns, const float *__restrict__ win,
                                           const float *__restrict__ delta, int nwin, int num_table, double ratio,
                                           float *__restrict__ out, int ldo) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ldo) return;
    const int Nb = clamp_count(ns[b], N);
    if (t >= (int)((double)Nb * ratio)) {
        out[(long)b * ldo + t] = 0.f;
        return;
    }
    out[(long)b * ldo + t] = kaiser_sample(x + (long)b * N, Nb, t, win, delta, nwin, num_table, ratio);
}
hipError_t launch_resample_kaiser_lens(const float *x, int B, int N, const int *ns, const float *win, const float *delta, int nwin,
                                       int num_table, double ratio, float *out, int ldo, hipStream_t s) {
    hipLaunchKernelGGL(resample_kaiser_len_kernel, dim3((ldo + 255) / 256, B), dim3(256), 0, s, x, N, ns, win, delta, nwin, num_table,
                       ratio, out, ldo);
    return hipGetLastError();
}

// frames[b] = resampled length of recording b / hop + 1: the row table of the masked mel and DCT GEMMs (ConvParams::lens)
__global__ void mfcc_frames_kernel(const int *__restrict__ ns, int B, int N, int norig, int nnew, int hop, int *__restrict__ frames) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) frames[b] = resampled_len_of(clamp_count(ns[b], N), norig, nnew) / hop + 1;
}
hipError_t launch_mfcc_frames(const int *ns, int B, int N, int norig, int nnew, int hop, int *frames, hipStream_t s) {
    hipLaunchKernelGGL(mfcc_frames_kernel, dim3((B + 255) / 256), dim3(256), 0, s, ns, B, N, norig, nnew, hop, frames);
    return hipGetLastError();
}

// x: rows of N samples at the OUTPUT rate (N = the resampled length of the padded input width); recording b holds
// ceil(ns[b] nnew / norig) of them.  Workgroup (b, t) of a (B, T) grid: the frame of stft_power_kernel with the reflect index on the
// recording's own length, or a zero row for t at or beyond the recording's own frame count (no FFT)
__global__ __launch_bounds__(256) void stft_power_len_kernel(const float *__restrict__ x, int N, int T, const int *__restrict__ ns, int norig,
                                                             int nnew, int hop, const float *__restrict__ win,
                                                             const f32x2 *__restrict__ tw1024, const f32x2 *__restrict__ tw2048,
                                                             float *__restrict__ pw, int ldp) {
    const long row = blockIdx.x;   // b * T + t
    const int b = (int)(row / T), t = (int)(row - (long)b * T);
    const int Nb = clamp_count(resampled_len_of(ns[b], norig, nnew), N);
    float *out = pw + row * ldp;
    if (t >= Nb / hop + 1) {
        for (int k = threadIdx.x; k < ldp; k += 256) out[k] = 0.f;
        return;
    }
    const float *xb = x + (long)b * N;
    auto sample = [&](int n) {
        int i = t * hop + n - 1024;
        if (i < 0) i = -i;
        if (i >= Nb) i = 2 * (Nb - 1) - i;
        i = i < 0 ? 0 : (i >= Nb ? Nb - 1 : i);
        return xb[i] * win[n];
    };
    stft_frame_power(sample, tw1024, tw2048, out, ldp);
}
hipError_t launch_stft_power_lens(const float *x, int B, int N, int T, const int *ns, int norig, int nnew, int hop, const float *win,
                                  const float *tw1024, const float *tw2048, float *pw, int ldp, hipStream_t s) {
    hipLaunchKernelGGL(stft_power_len_kernel, dim3((unsigned)((long)B * T)), dim3(256), 0, s, x, N, T, ns, norig, nnew, hop, win,
                       reinterpret_cast<const f32x2 *>(tw1024), reinterpret_cast<const f32x2 *>(tw2048), pw, ldp);
    return hipGetLastError();
}

// one workgroup per recording, rows of `width` values, T rows per recording of which frames[b] are its own: decibels, the maximum and the
// clamp over those rows only; the rows beyond are written as 0 (a second time in ts_mfcc_forward_mixed, whose masked mel GEMM has stored
// zeros there already: the kernel states its own contract and does not lean on its caller's)
__global__ __launch_bounds__(256) void db_topdb_len_kernel(float *__restrict__ mel, int T, int width, const int *__restrict__ frames,
                                                           float top_db) {
    __shared__ float sm[4];
    float *p = mel + (long)blockIdx.x * T * width;
    const long per_clip = (long)clamp_count(frames[blockIdx.x], T) * width, padded = (long)T * width;
    float mx = -INFINITY;
    for (long i = threadIdx.x; i < per_clip; i += 256) {
        const float v = db_of(p[i]);
        p[i] = v;
        mx = fmaxf(mx, v);
    }
    const float lo = block_max_256(mx, sm) - top_db;
    for (long i = threadIdx.x; i < per_clip; i += 256) p[i] = fmaxf(p[i], lo);
    for (long i = per_clip + threadIdx.x; i < padded; i += 256) p[i] = 0.f;
}
hipError_t launch_db_topdb_lens(float *mel, int B, int T, int width, const int *frames, float top_db, hipStream_t s) {
    hipLaunchKernelGGL(db_topdb_len_kernel, dim3(B), dim3(256), 0, s, mel, T, width, frames, top_db);
    return hipGetLastError();
}

// the maximum db_topdb_len_kernel clamps at, and nothing else: out[b] = max over the recording's own rows of 10 log10(max(x, 1e-10)); mel is
// only read (ts_mfcc_peak_db_mixed)
__global__ __launch_bounds__(256) void db_peak_len_kernel(const float *__restrict__ mel, int T, int width, const int *__restrict__ frames,
                                                          float *__restrict__ out) {
    __shared__ float sm[4];
    const float *p = mel + (long)blockIdx.x * T * width;
    const long per_clip = (long)clamp_count(frames[blockIdx.x], T) * width;
    float mx = -INFINITY;
    for (long i = threadIdx.x; i < per_clip; i += 256) mx = fmaxf(mx, db_of(p[i]));
    mx = block_max_256(mx, sm);
    if (threadIdx.x == 0) out[blockIdx.x] = mx;
}
hipError_t launch_db_peak_lens(const float *mel, int B, int T, int width, const int *frames, float *out, hipStream_t s) {
    hipLaunchKernelGGL(db_peak_len_kernel, dim3(B), dim3(256), 0, s, mel, T, width, frames, out);
    return hipGetLastError();
}

// ---- wav sessions (ts_mfcc_stream_*, mfcc.cpp; talkshow_hip.h, "wav sessions"): the front end fed samples in chunks.  A session keeps,
// per slot, the input samples its next output still reads and the resampled samples its next frame still reads, each as the front of a row
// buffer that the call's new samples are appended to; the kernels index those rows by ABSOLUTE sample index (the index the one-shot kernels
// use) minus the absolute index of the row's first element.  Every value comes from the body the one-shot kernel runs on the whole recording:
// the chunking moves WHEN a value is computed, never how. ----

// dst[b][i] = src[b][off + i], i < len: appends a call's samples to a row buffer and carries a buffer's tail over to its twin
__global__ void stream_rows_copy_kernel(const float *__restrict__ src, long lds, long off, int len, float *__restrict__ dst, long ldd) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < len) dst[b * ldd + i] = src[b * lds + off + i];
}
hipError_t launch_stream_rows_copy(const float *src, long lds, long off, int len, float *dst, long ldd, int B, hipStream_t s) {
    if (len < 1) return hipSuccess;
    hipLaunchKernelGGL(stream_rows_copy_kernel, dim3((len + 255) / 256, B), dim3(256), 0, s, src, lds, off, len, dst, ldd);
    return hipGetLastError();
}

// outputs j in [j_lo, j_hi) of resample_polyphase_kernel over a recording of which samples [x0, n) sit in x (rows of ldx, element 0 = sample
// x0); n = the samples received so far, or the recording's length at the flush: a tap at or beyond n reads as zero, as beyond the clip.
// An output is asked for only once its taps below n are all at or beyond x0.  out: rows of ldo, element 0 = output o0
__global__ void resample_polyphase_stream_kernel(const float *__restrict__ x, long ldx, long x0, long n, const float *__restrict__ kern,
                                                 int norig, int nnew, int width, int kw, float *__restrict__ out, long ldo, long o0, long j_lo,
                                                 long j_hi) {
    const int b = blockIdx.y;
    const long j = j_lo + (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= j_hi) return;
    out[b * ldo + (j - o0)] = polyphase_sum(Taps<long>{x + b * ldx, x0, n}, j, kern, norig, nnew, width, kw);
}
__global__ __launch_bounds__(256) void resample_polyphase_lds_stream_kernel(const float *__restrict__ x, long ldx, long x0, long n,
                                                                            const float *__restrict__ kern, int norig, int nnew, int width,
                                                                            int kw, float *__restrict__ out, long ldo, long o0, long j_lo,
                                                                            long j_hi, int nwin) {
    const int b = blockIdx.y;
    const long j0 = j_lo + (long)blockIdx.x * 256;
    polyphase_stage(Taps<long>{x + b * ldx, x0, n}, j0, kern, norig, nnew, width, kw, nwin);
    const long j = j0 + threadIdx.x;
    if (j >= j_hi) return;
    out[b * ldo + (j - o0)] = polyphase_staged_sum(j0, j, norig, nnew, width, kw);
}
hipError_t launch_resample_polyphase_stream(const float *x, long ldx, long x0, long n, int B, const float *kern, int norig, int nnew, int width,
                                            int kw, float *out, long ldo, long o0, long j_lo, long j_hi, hipStream_t s) {
    if (j_hi <= j_lo) return hipSuccess;
    const unsigned blocks = (unsigned)((j_hi - j_lo + 255) / 256);
    const PolyphaseLds l = polyphase_lds(norig, nnew, kw);
    if (l.staged) {
        hipLaunchKernelGGL(resample_polyphase_lds_stream_kernel, dim3(blocks, B), dim3(256), l.bytes, s, x, ldx, x0, n, kern, norig, nnew, width,
                           kw, out, ldo, o0, j_lo, j_hi, l.nwin);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(resample_polyphase_stream_kernel, dim3(blocks, B), dim3(256), 0, s, x, ldx, x0, n, kern, norig, nnew, width, kw, out,
                       ldo, o0, j_lo, j_hi);
    return hipGetLastError();
}

// frames t0 .. t0 + F - 1 of stft_power_kernel over a recording of which resampled samples [x0, ..) sit in x (rows of ldx, element 0 = sample
// x0).  N = the recording's resampled length at the flush; before it, the count of final resampled samples, which every frame asked for lies
// below (so the right reflection is never taken).  Workgroup (b, f) of a (B, F) grid writes row b F + f of pw.
__global__ __launch_bounds__(256) void stft_power_stream_kernel(const float *__restrict__ x, long ldx, long x0, long N, int F, int t0, int hop,
                                                                const float *__restrict__ win, const f32x2 *__restrict__ tw1024,
                                                                const f32x2 *__restrict__ tw2048, float *__restrict__ pw, int ldp) {
    const long row = blockIdx.x;   // b * F + f
    const int b = (int)(row / F), t = t0 + (int)(row - (long)b * F);
    const float *xb = x + b * ldx;
    auto sample = [&](int n) {
        long i = (long)t * hop + n - 1024;
        if (i < 0) i = -i;
        if (i >= N) i = 2 * (N - 1) - i;
        i = i < 0 ? 0 : (i >= N ? N - 1 : i);
        i = i < x0 ? x0 : i;       // never taken by a frame the session asks for: keeps a wrong plan inside the row
        return xb[i - x0] * win[n];
    };
    stft_frame_power(sample, tw1024, tw2048, pw + row * ldp, ldp);
}
hipError_t launch_stft_power_stream(const float *x, long ldx, long x0, long N, int B, int F, int t0, int hop, const float *win,
                                    const float *tw1024, const float *tw2048, float *pw, int ldp, hipStream_t s) {
    if (F < 1) return hipSuccess;
    hipLaunchKernelGGL(stft_power_stream_kernel, dim3((unsigned)((long)B * F)), dim3(256), 0, s, x, ldx, x0, N, F, t0, hop, win,
                       reinterpret_cast<const f32x2 *>(tw1024), reinterpret_cast<const f32x2 *>(tw2048), pw, ldp);
    return hipGetLastError();
}

// decibels and the clamp of db_topdb_kernel on the F new rows of every slot (mel: row b F + f, 256 values), in place; one thread per mel band.
//   peak != null: the floor of every row is peak[b] - top_db (the recording's maximum, known beforehand); grid (B, any): rows f = blockIdx.y,
//                 blockIdx.y + gridDim.y, ...; run_max is not touched
//   peak == null: the floor of row f is (the maximum over the slot's rows so far, this one included) - top_db: a prefix maximum along time,
//                 carried in run_max[b] from call to call; grid (B, 1)
__global__ __launch_bounds__(256) void db_stream_kernel(float *__restrict__ mel, int F, const float *__restrict__ peak,
                                                        float *__restrict__ run_max, float top_db) {
    __shared__ float sm[2][4];
    const int b = blockIdx.x;
    float *p = mel + (long)b * F * 256 + threadIdx.x;
    if (peak) {
        const float lo = peak[b] - top_db;
        for (int f = blockIdx.y; f < F; f += gridDim.y) p[(long)f * 256] = fmaxf(db_of(p[(long)f * 256]), lo);
        return;
    }
    float run = run_max[b];
    for (int f = 0; f < F; ++f) {
        const float v = db_of(p[(long)f * 256]);
        run = fmaxf(run, block_max_256(v, sm[f & 1]));      // two buffers: one barrier per row
        const float lo = run - top_db;
        p[(long)f * 256] = fmaxf(v, lo);
    }
    if (threadIdx.x == 0) run_max[b] = run;
}
hipError_t launch_db_stream(float *mel, int B, int F, const float *peak, float *run_max, float top_db, hipStream_t s) {
    if (F < 1) return hipSuccess;
    hipLaunchKernelGGL(db_stream_kernel, dim3(B, peak ? (F < 64 ? F : 64) : 1), dim3(256), 0, s, mel, F, peak, run_max, top_db);
    return hipGetLastError();
}

}  // namespace ts
