// Staging kernels of the seamless body sessions (talkshow_hip.h, "seamless sessions"; body_stream.cpp has the session and the window
// arithmetic).  The arithmetic of a push stays in the existing engines: ts_audioenc_forward, the PixelCNN session, ts_vqvae_decode_pair.
// These kernels move rows around them so that a push has no host round trip and no overlapping copy:
//   stream_stage_mfcc_kernel   [tail | chunk] -> the encoder window and the next tail (the other half of the session's double buffer)
//   stream_emit_kernel         the step's codes -> the code ring, and the decoder window's two latent columns out of ring + step
//   stream_keep_rows_kernel    rows [r0, r0 + n) of every clip of a (B, R, W) block -> a dense (B, n, W) block
// All three are copies: grid-stride, one element per thread and round, no LDS; 16-byte loads and stores where a row is a whole number of
// float4 (64-wide MFCC rows, 256-wide audio rows, the int64 code pairs); the 129-wide pose rows go word by word.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace ts {

namespace {
constexpr int STAGE_THREADS = 256;
constexpr int STAGE_MAX_BLOCKS = 2048;   // 8 workgroups per CU: more only queue behind each other for a copy

inline int stage_blocks(long units) {
    const long b = (units + STAGE_THREADS - 1) / STAGE_THREADS;
    return (int)(b < 1 ? 1 : (b > STAGE_MAX_BLOCKS ? STAGE_MAX_BLOCKS : b));
}

// Frame j of the concatenation [tail (n_tail frames of clip b) | chunk (t frames of clip b)], as 16 float4
__device__ inline float4 concat_load(const float4 *tail, long tail_ld4, int n_tail, const float4 *chunk, int t, int b, int j, int q) {
    return j < n_tail ? tail[(long)b * tail_ld4 + (long)j * 16 + q] : chunk[((long)b * t + (j - n_tail)) * 16 + q];
}

// win (B, Tw, 64) = frames [0, Tw) of the concatenation; next (B, cap, 64) rows [0, n_next) = frames [next0, next0 + n_next).
// Tw <= n_tail + t and next0 + n_next <= n_tail + t (checked by the launcher); tail and next are different buffers.
__global__ __launch_bounds__(STAGE_THREADS) void stream_stage_mfcc_kernel(const float4 *__restrict__ tail, const float4 *__restrict__ chunk,
                                                                          float4 *__restrict__ win, float4 *__restrict__ next, int B,
                                                                          int n_tail, int t, int cap, int Tw, int next0, int n_next) {
    const long ld4 = (long)cap * 16;
    const long n_win = (long)B * Tw * 16, n_all = n_win + (long)B * n_next * 16;
    for (long u = (long)blockIdx.x * STAGE_THREADS + threadIdx.x; u < n_all; u += (long)gridDim.x * STAGE_THREADS) {
        if (u < n_win) {
            const int q = (int)(u % 16);
            const long f = u / 16;
            const int j = (int)(f % Tw), b = (int)(f / Tw);
            win[u] = concat_load(tail, ld4, n_tail, chunk, t, b, j, q);
        } else {
            const long v = u - n_win;
            const int q = (int)(v % 16);
            const long f = v / 16;
            const int j = (int)(f % n_next), b = (int)(f / n_next);
            next[(long)b * ld4 + (long)j * 16 + q] = concat_load(tail, ld4, n_tail, chunk, t, b, next0 + j, q);
        }
    }
}

// codes (B, n, 2): the rows [A, A + n) this call produced; ring (B, RC, 2), row r of a clip at slot r % RC.  Appends the n rows and gathers
// rows [v0, v0 + Hw) into lat_body / lat_hand (B, Hw).  A gathered row at or beyond A is read from `codes`, an earlier one from the ring, so
// no thread reads a slot another writes in this launch (A + n - v0 <= RC: checked by the launcher).
__global__ __launch_bounds__(STAGE_THREADS) void stream_emit_kernel(const longlong2 *__restrict__ codes, longlong2 *__restrict__ ring,
                                                                    long long *__restrict__ lat_body, long long *__restrict__ lat_hand, int B,
                                                                    int n, int A, int RC, int v0, int Hw) {
    const long n_app = (long)B * n, n_all = n_app + (long)B * Hw;
    for (long u = (long)blockIdx.x * STAGE_THREADS + threadIdx.x; u < n_all; u += (long)gridDim.x * STAGE_THREADS) {
        if (u < n_app) {
            const int i = (int)(u % n), b = (int)(u / n);
            ring[(long)b * RC + (A + i) % RC] = codes[u];
        } else {
            const long v = u - n_app;
            const int h = (int)(v % Hw), b = (int)(v / Hw);
            const int r = v0 + h;
            const longlong2 c = r >= A ? codes[(long)b * n + (r - A)] : ring[(long)b * RC + r % RC];
            lat_body[v] = c.x;
            lat_hand[v] = c.y;
        }
    }
}

// dst (B, n, W) = rows [r0, r0 + n) of src (B, R, W); T = float4 (W counted in float4) or float
template <class T>
__global__ __launch_bounds__(STAGE_THREADS) void stream_keep_rows_kernel(const T *__restrict__ src, T *__restrict__ dst, int B, int R, int r0,
                                                                         int n, int W) {
    const long per = (long)n * W, n_all = (long)B * per;
    for (long u = (long)blockIdx.x * STAGE_THREADS + threadIdx.x; u < n_all; u += (long)gridDim.x * STAGE_THREADS) {
        const long b = u / per, e = u % per;
        dst[u] = src[(b * R + r0) * W + e];
    }
}

// dst (S, n, W4) = rows [r0, r0 + n) of stream map[s] of src (E, R, W4), W4 counted in float4: the kept audio rows of every encoder
// stream to the chain slots that hear it (a source may serve several slots: a shadow on its clip's audio).  map holds values in [0, E)
// (the session checks them on the host at open).  No scratch, one float4 per thread and round
__global__ __launch_bounds__(STAGE_THREADS) void stream_spread_rows_kernel(const float4 *__restrict__ src, float4 *__restrict__ dst,
                                                                           const int32_t *__restrict__ map, int S, int R, int r0, int n,
                                                                           int W4) {
    const long per = (long)n * W4, n_all = (long)S * per;
    for (long u = (long)blockIdx.x * STAGE_THREADS + threadIdx.x; u < n_all; u += (long)gridDim.x * STAGE_THREADS) {
        const long sl = u / per, e = u % per;
        dst[u] = src[((long)map[sl] * R + r0) * W4 + e];
    }
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

hipError_t launch_stream_stage_mfcc(const float *tail, const float *chunk, float *win, float *next, int B, int n_tail, int t, int cap, int Tw,
                                    int next0, int n_next, hipStream_t s) {
    if (B < 1 || n_tail < 0 || t < 0 || Tw < 0 || n_next < 0 || next0 < 0 || n_tail > cap || n_next > cap || Tw > n_tail + t ||
        next0 + n_next > n_tail + t || (t > 0 && !chunk) || tail == next || !aligned16(tail) || !aligned16(chunk) || !aligned16(win) ||
        !aligned16(next))
        return hipErrorInvalidValue;
    const long units = ((long)B * Tw + (long)B * n_next) * 16;
    if (units == 0) return hipSuccess;
    stream_stage_mfcc_kernel<<<stage_blocks(units), STAGE_THREADS, 0, s>>>(
        reinterpret_cast<const float4 *>(tail), reinterpret_cast<const float4 *>(chunk), reinterpret_cast<float4 *>(win),
        reinterpret_cast<float4 *>(next), B, n_tail, t, cap, Tw, next0, n_next);
    return hipGetLastError();
}

hipError_t launch_stream_emit(const int64_t *codes, int64_t *ring, int64_t *lat_body, int64_t *lat_hand, int B, int n, int A, int RC, int v0,
                              int Hw, hipStream_t s) {
    if (B < 1 || n < 0 || Hw < 0 || A < 0 || v0 < 0 || RC < 1 || v0 > A || A + n - v0 > RC || v0 + Hw > A + n || (n > 0 && !codes) ||
        (Hw > 0 && (!lat_body || !lat_hand)) || !ring || !aligned16(codes) || !aligned16(ring))
        return hipErrorInvalidValue;
    const long units = (long)B * n + (long)B * Hw;
    if (units == 0) return hipSuccess;
    stream_emit_kernel<<<stage_blocks(units), STAGE_THREADS, 0, s>>>(reinterpret_cast<const longlong2 *>(codes),
                                                                      reinterpret_cast<longlong2 *>(ring),
                                                                      reinterpret_cast<long long *>(lat_body),
                                                                      reinterpret_cast<long long *>(lat_hand), B, n, A, RC, v0, Hw);
    return hipGetLastError();
}

hipError_t launch_stream_keep_rows(const float *src, float *dst, int B, int R, int r0, int n, int W, hipStream_t s) {
    if (B < 1 || R < 1 || W < 1 || r0 < 0 || n < 0 || r0 + n > R || !src || (n > 0 && !dst)) return hipErrorInvalidValue;
    const long units = (long)B * n * W;
    if (units == 0) return hipSuccess;
    if (W % 4 == 0 && aligned16(src) && aligned16(dst))
        stream_keep_rows_kernel<float4><<<stage_blocks(units / 4), STAGE_THREADS, 0, s>>>(
            reinterpret_cast<const float4 *>(src), reinterpret_cast<float4 *>(dst), B, R, r0, n, W / 4);
    else
        stream_keep_rows_kernel<float><<<stage_blocks(units), STAGE_THREADS, 0, s>>>(src, dst, B, R, r0, n, W);
    return hipGetLastError();
}

hipError_t launch_stream_spread_rows(const float *src, float *dst, const int32_t *map, int S, int E, int R, int r0, int n, int W,
                                     hipStream_t s) {
    if (S < 1 || E < 1 || R < 1 || W < 4 || W % 4 || r0 < 0 || n < 0 || r0 + n > R || !src || !map || (n > 0 && !dst) || !aligned16(src) ||
        !aligned16(dst))
        return hipErrorInvalidValue;
    const long units = (long)S * n * (W / 4);
    if (units == 0) return hipSuccess;
    stream_spread_rows_kernel<<<stage_blocks(units), STAGE_THREADS, 0, s>>>(reinterpret_cast<const float4 *>(src),
                                                                             reinterpret_cast<float4 *>(dst), map, S, R, r0, n, W / 4);
    return hipGetLastError();
}

}  // namespace ts
