// Code tables of the PixelCNN chain: the two launches of a code row that multiply nothing but embeddings of codes that are
// already known — slot V0 of the vertical stack (W2 . E[r-1] with its riders W1 . E[r-1], W0 . E[r-1]) and hg_0 of column 1
// (wh[0] . emb[code(r, 0)]) — as lookups.  With V codes each product takes one of V values per weight matrix.
//
// The chain's contract is BIT identity: a clip's result must not depend on the kernel that served its stage.  The chain
// kernels (skinny_gemm.hip, skinny_wide.hip) cut K into W slices (the split-K waves' shares: q-steps [Q w / W, Q (w + 1) / W)
// of 16 k, Q = K / 16, W from plan_skinny), run every slice as a chain of v_mfma_f32_16x16x4_f32 from zero with k ascending,
// add the slice sums in index order and then the epilogue terms.  The tables hold slice sums made by the same instruction
// in the same order, and the stage kernel adds them in the same order:
//   * a code that covers the slices FIRST in the order (column 0 of V0, the one code of hg_0) contributes one row per
//     code: the prefix ((s_0 + s_1) + ...) of its slices;
//   * a code whose slices are added one by one onto that running total (column 1 of V0) contributes one row per slice.
// The tables depend on the weights alone: built once per model (pixelcnn.cpp), shared by every stream and call.
#include "skinny_desc.h"

namespace ts {

// out[code][n] = the sum, in index order, of slices [s0, s1) of W[n][.] . E[code][. - kcol]   (one row set of a table)
// One wave per 16 channels x 16 codes: weights as the A operand, embeddings as B, the accumulator from zero per slice —
// the wide kernel's operand roles, lane (i, g) supplying k = 16 q + 4 g + e to the e-th instruction of a q-step.
__global__ __launch_bounds__(64) void code_table_build_kernel(const CodeTableBuild p) {
    const int lane = threadIdx.x, li = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16, c0 = blockIdx.y * 16;
    const int code = c0 + li;
    const bool code_ok = code < p.V;
    const float *wrow = p.W + (long)(n0 + li) * p.ldw + lg * 4;
    const float *erow = p.emb + (long)(code_ok ? code : 0) * p.D + lg * 4 - p.kcol;
    const int Q = p.K >> 4;
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    for (int s = p.s0; s < p.s1; ++s) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const int qb = (Q * s) / p.waves, qe = (Q * (s + 1)) / p.waves;
        for (int q = qb; q < qe; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4 *>(wrow + q * 16);
            const f32x4 b = code_ok ? *reinterpret_cast<const f32x4 *>(erow + q * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
        }
        if (s == p.s0) tot = acc;   // the chain kernels' red[0] + red[1] + ...: the first slice is taken, not added to zero
        else tot += acc;
    }
    // D[i = channel lg * 4 + r][j = code li]
    if (code_ok) *reinterpret_cast<f32x4 *>(p.out + (long)code * p.N + n0 + lg * 4) = tot;
}

hipError_t launch_code_table_build(const CodeTableBuild &p, hipStream_t stream) {
    if (p.N % 16 || p.K % 16 || p.V < 1 || p.waves < 1 || p.s0 < 0 || p.s1 > p.waves || p.s0 >= p.s1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(code_table_build_kernel, dim3(p.N / 16, (p.V + 15) / 16), dim3(64), 0, stream, p);
    return hipGetLastError();
}

// ---- the stage ----------------------------------------------------------------------------------------------------------
// One thread owns 4 consecutive "tanh" channels of one clip and their 4 "sigmoid" partners (gateD channels further): every
// access is a 16-byte vector and the gate needs no exchange.  The sums follow the chain kernels' epilogue to the letter:
//   tot = (((P[c0] + S_1[c1]) + S_2[c1]) + ...)            slice sums in index order (a negative code: the zero row, +0.0)
//   v   = tot + (((bias + add1) + add2) + 0)               absent terms are +0.0, as the descriptor kernels read them
//   pre = v;  out = gate_act(v + cls, partner + cls)
// and a rider (a linear problem without terms) is tot + 0.0.
__device__ __forceinline__ f32x4 code_table_sum(const float *tab, long set_stride, int nsets, long row0, long row1, int n) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 x[CODE_TABLE_MAX_SETS];
#pragma unroll
    for (int s = 0; s < CODE_TABLE_MAX_SETS; ++s) {   // every load goes out before the first add
        const long row = s == 0 ? row0 : row1;
        x[s] = (s < nsets && row >= 0) ? *reinterpret_cast<const f32x4 *>(tab + s * set_stride + row + n) : zero;
    }
    f32x4 tot = x[0];
#pragma unroll
    for (int s = 1; s < CODE_TABLE_MAX_SETS; ++s)
        if (s < nsets) tot += x[s];
    return tot;
}

__global__ __launch_bounds__(256) void code_table_stage_kernel(const CodeTableStage p) {
    const int per_clip = p.N >> 3;                    // threads of a clip: N / 2 tanh channels, 4 each
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int m = (int)(gid / per_clip);
    if (m >= p.M) return;
    const int t = (int)(gid - (long)m * per_clip);
    const int per_group = p.gateD >> 2;
    const int group = t / per_group, ch = (t - group * per_group) << 2;
    const int nt = group * 2 * p.gateD + ch, ns = nt + p.gateD;   // weight-row numbering: tanh, sigmoid partner

    const int c0 = p.tok0[(long)m * p.tok_stride];
    const int c1 = p.nsets > 1 ? p.tok1[(long)m * p.tok_stride] : -1;
    const long row0 = c0 >= 0 ? (long)c0 * p.N : -1, row1 = c1 >= 0 ? (long)c1 * p.N : -1;

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    auto ld = [&](const float *base, long off) { return base ? *reinterpret_cast<const f32x4 *>(base + off) : zero; };
    f32x4 tot[2], rid[2][2];
    tot[0] = code_table_sum(p.tab[0], p.set_stride, p.nsets, row0, row1, nt);
    tot[1] = code_table_sum(p.tab[0], p.set_stride, p.nsets, row0, row1, ns);
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (p.rider[k]) {
            rid[k][0] = code_table_sum(p.tab[1 + k], p.set_stride, p.nsets, row0, row1, nt);
            rid[k][1] = code_table_sum(p.tab[1 + k], p.set_stride, p.nsets, row0, row1, ns);
        }
    f32x4 v[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int n = h ? ns : nt;
        const f32x4 t0 = ld(p.bias, n), t1 = ld(p.add1, (long)m * p.add1_stride + n), t2 = ld(p.add2, (long)m * p.add2_stride + n);
        v[h] = tot[h] + (((t0 + t1) + t2) + zero);
        if (p.pre) {
            const long ip = (long)m * p.pre_stride + n;
            *reinterpret_cast<f32x4 *>(p.pre + (p.pre_tw ? tiled_index(ip, p.pre_tw) : ip)) = v[h];
        }
        v[h] += ld(p.cls, (long)m * p.cls_ld + (n % p.cls_ld));
    }
    f32x4 g;
#pragma unroll
    for (int r = 0; r < 4; ++r) g[r] = gate_act(v[0][r], v[1][r]);
    const long io = (long)m * p.out_stride + group * p.gateD + ch;
    *reinterpret_cast<f32x4 *>(p.out + (p.out_tw ? tiled_index(io, p.out_tw) : io)) = g;
#pragma unroll
    for (int k = 0; k < 2; ++k)
        if (p.rider[k]) {
            float *q = p.rider[k] + (long)m * p.rider_stride;
            *reinterpret_cast<f32x4 *>(q + nt) = rid[k][0] + (((zero + zero) + zero) + zero);
            *reinterpret_cast<f32x4 *>(q + ns) = rid[k][1] + (((zero + zero) + zero) + zero);
        }
}

hipError_t launch_code_table_stage(const CodeTableStage &p, hipStream_t stream) {
    auto al16 = [](const void *q) { return ((uintptr_t)q & 15) == 0; };
    if (p.M < 1 || p.gateD < 4 || p.gateD % 4 || p.N % (2 * p.gateD) || p.nsets < 1 || p.nsets > CODE_TABLE_MAX_SETS || !p.tab[0] || !p.tok0 ||
        (p.nsets > 1 && !p.tok1) || !p.out || p.cls_ld < 4 || p.cls_ld % 4 || p.set_stride % 4)
        return hipErrorInvalidValue;
    if (!al16(p.tab[0]) || !al16(p.tab[1]) || !al16(p.tab[2]) || !al16(p.bias) || !al16(p.add1) || !al16(p.add2) || !al16(p.cls) || !al16(p.pre) ||
        !al16(p.out) || !al16(p.rider[0]) || !al16(p.rider[1]))
        return hipErrorInvalidValue;
    if (p.add1_stride % 4 || p.add2_stride % 4 || p.pre_stride % 4 || p.out_stride % 4 || p.rider_stride % 4) return hipErrorInvalidValue;
    if ((p.rider[0] && !p.tab[1]) || (p.rider[1] && !p.tab[2])) return hipErrorInvalidValue;
    const long threads = (long)p.M * (p.N >> 3);
    hipLaunchKernelGGL(code_table_stage_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError();
}

}  // namespace ts
