// Winograd F(4,3) lowering of the wide stride-1 k = 3 C -> C layers (models.cpp::run_stack_n): the three element-wise transforms around
// the six C x C GEMMs that conv_gemm_f32 runs as batched problems.  Standard matrices, interpolation points 0, +-1, +-2, inf
// (Lavin & Gray, "Fast Algorithms for Convolutional Neural Networks", 2015):
//   G  = [[1/4,0,0],[-1/6,-1/6,-1/6],[-1/6,1/6,-1/6],[1/24,1/12,1/6],[1/24,-1/12,1/6],[0,0,1]]         (weights, host: wino_transform_weights)
//   Bt = [[4,0,-5,0,1,0],[0,-4,-4,1,1,0],[0,4,-4,-1,1,0],[0,-2,-1,2,1,0],[0,2,-1,-2,1,0],[0,4,0,-5,0,1]]   (input)
//   At = [[1,1,1,1,1,0],[0,1,-1,2,-2,0],[0,1,1,4,4,0],[0,1,-1,8,-8,1]]                                   (output)
// Tiles are per clip: tile j of clip b covers output rows 4j .. 4j + 3 and reads input rows 4j - 1 .. 4j + 4 of that clip; rows outside
// [0, L_b) read as zeros, L_b = the clip's own length ((lens[b] >> shr) << shl in a mixed pass, else L).  J = ceil(L / 4) tiles per clip.
//   V (6, B J, C): V_i[b J + j] = sum_k Bt[i][k] x[b][4j - 1 + k]          O (6, B J, C) = the GEMMs' outputs V_i U_i^T
//   y[b][4j + r] = act(sum_i At[r][i] O_i[b J + j] + bias (+ res)); rows in [L_b, L) are stored as zeros, like the masked conv epilogue's.
//
// SUMMATION ORDER (pinned by tests/test_gpu_wino.py against a numpy restatement, bit for bit).  Every line is evaluated left to right, one
// IEEE fp32 operation per sign or product, no fused multiply-add (fp contract off):
//   V0 = 4 d0 - 5 d2 + d4            V1 = -4 d1 - 4 d2 + d3 + d4 = ((d3 - 4 d1) - 4 d2) + d4      V2 = ((4 d1 - 4 d2) - d3) + d4
//   V3 = ((2 d3 - 2 d1) - d2) + d4   V4 = ((2 d1 - d2) - 2 d3) + d4                               V5 = (4 d1 - 5 d3) + d5
//   y0 = (((m0 + m1) + m2) + m3) + m4          y1 = ((m1 - m2) + 2 m3) - 2 m4
//   y2 = ((m1 + m2) + 4 m3) + 4 m4             y3 = (((m1 - m2) + 8 m3) - 8 m4) + m5
//   then v = y + bias, v = v + res (if given), v = act(v).
// wino_out_in evaluates exactly these expressions for the six rows a tile of the next layer reads, so it equals wino_out followed by
// wino_in bit for bit; the intermediate y is never stored.
// wino_codes (the decoder's first stack, whose input rows are rows of the aft_vq table) writes the first layer's O straight from the codes:
//   O_i[b J + j] = sum_k Bt[i][k] T_i[code[b][4j - 1 + k]], T_i = table U_i^T, in V_i's expression with T_i[c_k] in place of d_k
// (pinned by tests/test_gpu_vq_tables.py).  It rounds otherwise than wino_in followed by the GEMMs, within the same fp32 bound.
#include "kernels.h"
#include "conv_tile.h"

namespace ts {

namespace {

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, f32x4 v) { *reinterpret_cast<f32x4 *>(p) = v; }

__device__ __forceinline__ void wino_bt(const f32x4 (&d)[6], f32x4 (&v)[6]) {
#pragma clang fp contract(off)
    v[0] = (4.f * d[0] - 5.f * d[2]) + d[4];
    v[1] = ((d[3] - 4.f * d[1]) - 4.f * d[2]) + d[4];
    v[2] = ((4.f * d[1] - 4.f * d[2]) - d[3]) + d[4];
    v[3] = ((2.f * d[3] - 2.f * d[1]) - d[2]) + d[4];
    v[4] = ((2.f * d[1] - d[2]) - 2.f * d[3]) + d[4];
    v[5] = (4.f * d[1] - 5.f * d[3]) + d[5];
}

// row r (0 .. 3) of At m
__device__ __forceinline__ f32x4 wino_at_row(const f32x4 (&m)[6], const int r) {
#pragma clang fp contract(off)
    if (r == 0) return (((m[0] + m[1]) + m[2]) + m[3]) + m[4];
    if (r == 1) return ((m[1] - m[2]) + 2.f * m[3]) - 2.f * m[4];
    if (r == 2) return ((m[1] + m[2]) + 4.f * m[3]) + 4.f * m[4];
    return (((m[1] - m[2]) + 8.f * m[3]) - 8.f * m[4]) + m[5];
}

__device__ __forceinline__ f32x4 wino_finish(f32x4 y, const f32x4 bias, const float *res, const int act) {
#pragma clang fp contract(off)
    f32x4 v = y + bias;
    if (res) v = v + ld4(res);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float e = v[q];
        if (act == 1) e = e >= 0.f ? e : e * 0.2f;
        else if (act == 2) e = e > 0.f ? e : 0.f;
        else if (act == 3) e = gelu_fast(e);
        v[q] = e;
    }
    return v;
}

// what every thread of the three kernels is: 4 channels of tile (b, j) of network blockIdx.y
struct WinoItem {
    int net, b, j, c, Lb;
    long row;   // b J + j
    bool ok;
};
__device__ __forceinline__ WinoItem wino_item(const WinoParams &p) {
    WinoItem w;
    const int c4 = p.C >> 2;
    unsigned bx = blockIdx.x;
    w.net = blockIdx.y;
    if (p.deal) {   // 1-D grid of nnet * deal workgroups; ids of equal residue mod 8 share an XCD: XCD x takes the x-th contiguous eighth
        const unsigned total = gridDim.x, q = total >> 3, r = total & 7, x = bx & 7;
        const unsigned g = x * q + (x < r ? x : r) + (bx >> 3);
        w.net = g >= (unsigned)p.deal;
        bx = g - (w.net ? p.deal : 0);
    }
    const long idx = (long)bx * blockDim.x + threadIdx.x;
    w.row = idx / c4;
    w.c = (int)(idx - w.row * c4) << 2;
    w.ok = w.row < (long)p.B * p.J;
    w.b = (int)(w.row / p.J);
    w.j = (int)(w.row - (long)w.b * p.J);
    w.Lb = p.L;
    if (w.ok && p.lens) {
        const int l = (p.lens[w.b] >> p.len_shr) << p.len_shl;
        w.Lb = l < p.L ? l : p.L;
    }
    return w;
}

__device__ __forceinline__ void wino_load_tile(const float *O, const long comp_stride, const long row, const int C, const int c, f32x4 (&m)[6]) {
#pragma unroll
    for (int i = 0; i < 6; ++i) m[i] = ld4(O + i * comp_stride + row * C + c);
}

__global__ __launch_bounds__(256) void wino_in_kernel(const WinoParams p) {
    const WinoItem w = wino_item(p);
    if (!w.ok) return;
    const float *x = p.x[w.net] + (long)w.b * p.L * p.C + w.c;
    f32x4 d[6], v[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int t = 4 * w.j - 1 + k;
        d[k] = t >= 0 && t < w.Lb ? ld4(x + (long)t * p.C) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    wino_bt(d, v);
    const long cs = (long)p.B * p.J * p.C;
    float *V = p.V[w.net] + w.row * p.C + w.c;
#pragma unroll
    for (int i = 0; i < 6; ++i) st4(V + i * cs, v[i]);
}

__global__ __launch_bounds__(256) void wino_out_kernel(const WinoParams p) {
    const WinoItem w = wino_item(p);
    if (!w.ok) return;
    const long cs = (long)p.B * p.J * p.C;
    f32x4 m[6];
    wino_load_tile(p.O[w.net], cs, w.row, p.C, w.c, m);
    const f32x4 bias = ld4(p.bias[w.net] + w.c);
    const float *res = p.res[w.net];
    float *y = p.y[w.net] + (long)w.b * p.L * p.C + w.c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = 4 * w.j + r;
        if (t >= p.L) break;
        f32x4 v{0.f, 0.f, 0.f, 0.f};
        if (t < w.Lb) v = wino_finish(wino_at_row(m, r), bias, res ? res + ((long)w.b * p.L + t) * p.C + w.c : nullptr, p.act);
        st4(y + (long)t * p.C, v);
    }
}

__global__ __launch_bounds__(256) void wino_out_in_kernel(const WinoParams p) {
    const WinoItem w = wino_item(p);
    if (!w.ok) return;
    const long cs = (long)p.B * p.J * p.C;
    const float *O = p.O[w.net];
    const f32x4 bias = ld4(p.bias[w.net] + w.c);
    const f32x4 zero{0.f, 0.f, 0.f, 0.f};
    f32x4 m[6], d[6], v[6];
    // y[4j - 1]: row 3 of tile j - 1
    d[0] = zero;
    if (w.j > 0 && 4 * w.j - 1 < w.Lb) {
        wino_load_tile(O, cs, w.row - 1, p.C, w.c, m);
        d[0] = wino_finish(wino_at_row(m, 3), bias, nullptr, p.act);
    }
    // y[4j .. 4j + 3]: this tile
    wino_load_tile(O, cs, w.row, p.C, w.c, m);
#pragma unroll
    for (int r = 0; r < 4; ++r) d[1 + r] = 4 * w.j + r < w.Lb ? wino_finish(wino_at_row(m, r), bias, nullptr, p.act) : zero;
    // y[4j + 4]: row 0 of tile j + 1
    d[5] = zero;
    if (w.j + 1 < p.J && 4 * w.j + 4 < w.Lb) {
        wino_load_tile(O, cs, w.row + 1, p.C, w.c, m);
        d[5] = wino_finish(wino_at_row(m, 0), bias, nullptr, p.act);
    }
    wino_bt(d, v);
    float *V = p.V[w.net] + w.row * p.C + w.c;
#pragma unroll
    for (int i = 0; i < 6; ++i) st4(V + i * cs, v[i]);
}

// wino_in and the six GEMMs of a layer whose input rows are rows of a table (the decoder's first stack: x[b][t] = aft_table[code[b][t]]).
// The GEMMs are linear in x, so O_i = sum_k Bt[i][k] T_i[code(4j - 1 + k)] with T_i = table U_i^T made once per network; only the 22
// non-zero entries of Bt are read.  wino_bt's expressions and order, T_i[c_k] in place of d[k].
// A code outside [0, ncode) reads no table and counts as the zero row here, silently; the gather beside this launch still writes that row
// of x as NaN (vq.hip::gather_rows_kernel, "memory-safe and loud"), which reaches the stack's output through the tail's residual: the bad
// code shows as NaN in its own four pose rows, no longer in every row its tiles' GEMMs touched.
__global__ __launch_bounds__(256) void wino_codes_kernel(const WinoParams p) {
#pragma clang fp contract(off)
    const WinoItem w = wino_item(p);
    if (!w.ok) return;
    const int ncode = p.ncode[w.net];
    const int64_t *codes = p.codes[w.net] + (long)w.b * p.L;
    long off[6];   // of code row k within one T_i, -1: the zero row
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int t = 4 * w.j - 1 + k;
        off[k] = -1;
        if (t >= 0 && t < w.Lb) {
            const int64_t r = codes[t];
            if (r >= 0 && r < ncode) off[k] = (long)r * p.C + w.c;
        }
    }
    const float *T = p.T[w.net];
    const long ts = (long)ncode * p.C;
    auto row = [&](const int i, const int k) { return off[k] >= 0 ? ld4(T + i * ts + off[k]) : f32x4{0.f, 0.f, 0.f, 0.f}; };
    f32x4 v[6];
    v[0] = (4.f * row(0, 0) - 5.f * row(0, 2)) + row(0, 4);
    v[1] = ((row(1, 3) - 4.f * row(1, 1)) - 4.f * row(1, 2)) + row(1, 4);
    v[2] = ((4.f * row(2, 1) - 4.f * row(2, 2)) - row(2, 3)) + row(2, 4);
    v[3] = ((2.f * row(3, 3) - 2.f * row(3, 1)) - row(3, 2)) + row(3, 4);
    v[4] = ((2.f * row(4, 1) - row(4, 2)) - 2.f * row(4, 3)) + row(4, 4);
    v[5] = (4.f * row(5, 1) - 5.f * row(5, 3)) + row(5, 5);
    const long cs = (long)p.B * p.J * p.C;
    float *O = p.Ow[w.net] + w.row * p.C + w.c;
#pragma unroll
    for (int i = 0; i < 6; ++i) st4(O + i * cs, v[i]);
}

}  // namespace

hipError_t launch_wino(int which, const WinoParams &p, hipStream_t stream) {
    if (p.nnet < 1 || p.nnet > 2 || p.B < 1 || p.L < 1 || p.C < 4 || (p.C & 3) || p.J != (p.L + 3) / 4 || p.act < 0 || p.act > 3 ||
        (p.lens && (p.len_shr < 0 || p.len_shl < 0)))
        return hipErrorInvalidValue;
    const long items = (long)p.B * p.J * (p.C >> 2);
    if (items + 255 >= (1l << 31)) return hipErrorInvalidValue;
    for (int n = 0; n < p.nnet; ++n) {
        const bool in = which == 0   ? p.x[n] && p.V[n]
                        : which == 1 ? p.O[n] && p.bias[n] && p.y[n]
                        : which == 2 ? p.O[n] && p.bias[n] && p.V[n]
                                     : p.codes[n] && p.T[n] && p.Ow[n] && p.ncode[n] > 0;
        if (!in) return hipErrorInvalidValue;
    }
    // wino_out_in reads its two neighbour tiles: consecutive workgroups on one XCD fetch an O row into one L2, not three.  Rests on what
    // ts_ctx_create probed (conv_sk_supported); the plain grid otherwise.  The same bits either way
    const unsigned nb = (unsigned)((items + 255) / 256);
    WinoParams q = p;
    q.deal = knobs().wino_deal && conv_sk_supported() ? (int)nb : 0;
    const dim3 grid = q.deal ? dim3(nb * p.nnet) : dim3(nb, p.nnet);
    if (which == 0) hipLaunchKernelGGL(wino_in_kernel, grid, dim3(256), 0, stream, q);
    else if (which == 1) hipLaunchKernelGGL(wino_out_kernel, grid, dim3(256), 0, stream, q);
    else if (which == 2) hipLaunchKernelGGL(wino_out_in_kernel, grid, dim3(256), 0, stream, q);
    else if (which == 3) hipLaunchKernelGGL(wino_codes_kernel, grid, dim3(256), 0, stream, q);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// host: U_i = sum_k G[i][k] g_k in double from the folded taps w (cout, cin, 3), each rounded once to fp32; out (6, npad, cin), rows at or
// beyond cout zero
void wino_transform_weights(const float *w, int cout, int cin, int npad, float *out) {
    static const double G[6][3] = {{1.0 / 4, 0, 0},          {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                   {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};
    for (int i = 0; i < 6; ++i)
        for (int o = 0; o < npad; ++o)
            for (int c = 0; c < cin; ++c) {
                double u = 0.0;
                if (o < cout) {
                    const float *g = w + ((size_t)o * cin + c) * 3;
                    u = G[i][0] * (double)g[0] + G[i][1] * (double)g[1] + G[i][2] * (double)g[2];
                }
                out[((size_t)i * npad + o) * cin + c] = (float)u;
            }
}

}  // namespace ts
