// Internal kernel-launch interface shared by the .hip kernel files and the host-side model code.
// Everything here is plain structs + launch functions; the public C ABI is include/talkshow_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ts {

struct Knobs;   // the TS_* test levers (below)

// ------------------------------------------------------------------------------------------------
// conv_gemm_f32: 1-D convolution / transposed convolution / pointwise linear as an implicit GEMM on the
// fp32 MFMA (v_mfma_f32_32x32x2_f32).  Activations are NLC ([b][t][c], row stride ld floats, c padded to
// a multiple of 32 with zeros).  One output row m = b*Lout + t gathers, per segment s, `len` channels
// starting at c0 of input row t*stride + d (zero if outside [0, Lin)); the packed weight row n holds the
// segments back to back (Ktot floats, K-contiguous), BatchNorm already folded in.
// ------------------------------------------------------------------------------------------------
struct ConvSeg {
    int d;    // input row shift of the first tap
    int c0;   // first input channel
    int len;  // channels per tap (multiple of 32)
    int ntap; // consecutive taps d, d+1, ... sharing c0/len (0 or 1 = a single tap); K of the segment = ntap*len
};

struct ConvGroup {
    const float *x;     // input  [B*Lin][ldx]
    const float *w;     // packed weights [Npad][Ktot]
    const float *bias;  // [Npad]
    const float *res;   // optional residual [M][ldr] added before the activation
    float *out;         // output [M][ldo], written at columns out_col0 .. out_col0+N-1
    int out_col0;
    int nseg;
    ConvSeg seg[4];
};

struct ConvParams {
    int M, Lout, Lin, stride;
    int ldx, ldo, ldr;
    int N;     // columns stored per group (weights/bias are padded to a multiple of 128 rows)
    int Ktot;
    int act;   // 0 none, 1 LeakyReLU(0.2), 2 ReLU, 3 GELU (erf)
    int ngroups;
    ConvGroup g[4];
    // optional extras (0 = off)
    int res_after_act;   // residual is added after the activation instead of before it
    long ldw;            // weight row stride in floats (0 = Ktot, packed)
    int w_rows;          // number of valid weight rows (0 = padded to the grid); rows beyond read as zero
    // batched mode (zdiv > 0): blockIdx.z = z0*zdiv + z1 indexes independent problems that share g[0]'s geometry;
    // pointers advance by z0*zs0 + z1*zs1 floats
    const float *zero;   // >= 64 KB of zeros (filled by the launcher): where halo / padding operand pointers are parked
    int zdiv;
    long x_zs0, x_zs1, w_zs0, w_zs1, o_zs0, o_zs1, b_zs1, r_zs0, r_zs1;
    int sk_ok;           // the caller accepts the ring engine's stream-K plan: results within fp32 rounding of the whole-tile plans, deterministic,
                         // but a row's bits depend on M (which tiles get split).  Set by the face generator only; the body path never sets it
    float *sk_ws;        // stream-K band of the ring engine (conv_gemm_ring.hip): partial accumulators, two 128 x 128 fp32 blocks per band workgroup,
    int *sk_flags;       // and one arrival counter per band tile (zero between launches); set by launch_conv_gemm_ring_sk
    int w_planes;        // conv_gemm_split, 2 planes only: the weights are plane images already (split_weight_planes): no split of B in the kernel
    int xcd_tiles;       // set by launch_conv_gemm_split (0 or the column-group width): 1-D grid, tiles dealt to the XCDs in blocks that share operands
    // length-masked rows (mixed passes: clips of different lengths padded into one batch; null = off, the kernels that run then are
    // the unmasked instantiations).  lens[b] = the clip's base length; GEMM row m = b * Lout + t is valid for t < (lens[b] >> len_shr) << len_shl.
    // The masked epilogue stores ZERO for every other row — the operand the gather parks for rows outside [0, Lin) of a clip run alone,
    // so the next layer's taps read the same values in both cases and a valid row's bits do not depend on the padding.
    const int *lens;
    int len_shr, len_shl;
};

// banded conv_gemm launch (conv_gemm.hip): rows [0, mt_big * 128) in 128 x 128 tiles = workgroups [0, first_small), the rows
// after them in mt_small row blocks of the small tile shape = workgroups [first_small, total)
struct ConvBands {
    int mt_big, mt_small, first_small, total;
};

// stream-K launch of the ring engine (conv_gemm_ring.hip), per problem: row tiles [0, mt_dp) of 128 rows as whole 128 x 128 tiles
// (dp8 dealt workgroup ids), the mt_sk row tiles after them as ONE list of (tile, 32-k stage) iterations cut into wsk equal runs,
// one workgroup each; `stages` = Ktot / 32
struct ConvSK {
    int mt_dp, mt_sk, dp8, wsk, stages;
};
// The band's run arithmetic, one definition for the kernel and the host-side test (ts_debug_conv_sk_run): Ts band tiles of `stages` stages;
// XCD c holds tiles [tlo(c), tlo(c + 1)); its w8 = wsk / 8 runs cut its iterations evenly.  All in band-iteration units (tile * stages + stage).
struct SkRuns {
    int Ts, stages, w8;
    __host__ __device__ int tlo(int c) const { return (int)((long)c * Ts / 8); }
    __host__ __device__ int xcd_of_tile(int tile) const {
        int c = (int)((long)tile * 8 / Ts);
        if (c > 7) c = 7;
        while (c < 7 && tlo(c + 1) <= tile) ++c;
        while (c > 0 && tlo(c) > tile) --c;
        return c;
    }
    __host__ __device__ int begin(int c, int r) const {   // first iteration of run r of XCD c (r == w8: one past its last)
        const int base = tlo(c) * stages, Ic = (tlo(c + 1) - tlo(c)) * stages;
        return base + (int)((long)r * Ic / w8);
    }
    __host__ __device__ int run_of(int c, int x) const {  // the run of XCD c that holds iteration x
        const int base = tlo(c) * stages, Ic = (tlo(c + 1) - tlo(c)) * stages;
        int r = (int)((long)(x - base) * w8 / Ic);
        while (r + 1 < w8 && begin(c, r + 1) <= x) ++r;
        while (r > 0 && begin(c, r) > x) --r;
        return r;
    }
};

hipError_t conv_sk_probe_xcd_map(int device);                   // host, once per device (ts_ctx_create): do workgroup ids of equal residue mod 8 share an XCD?
bool conv_sk_supported();                                       // ... the answer for the current device (false before the probe ran)
bool conv_gemm_plan_sk_shape(const ConvParams &p, ConvSK &sk); // host only, by shape: false = the layer has no partly filled last unit worth splitting
bool conv_sk_valid(const ConvParams &p, const ConvSK &sk);     // host only: sk covers p's row tiles, has one band workgroup per unit slot and no empty run
// host (models.cpp): per-stream scratch of the stream-K band — ws_floats floats + nflags zeroed ints, grown on demand, dropped with the stream
int conv_sk_workspace(hipStream_t s, size_t ws_floats, size_t nflags, float **ws, int **flags);

bool conv_gemm_plan_bands(const ConvParams &p, ConvBands &bd);  // host only: the bands of a layer given to 128 x 128 tiles (false: none — under one round, or whole rounds)
bool conv_taps48_takes(const ConvParams &p);   // host: would conv_taps48.hip take this layer as laid out?

// Which kernel runs a conv layer (conv_gemm.hip::plan_conv):
//   Reg         conv_gemm.hip, global -> VGPR -> LDS staging: one plain grid of bm x bn tiles (wm x wn per wave, bk-deep chunks)
//   RegBanded   conv_gemm.hip: 128 x 128 tiles for the whole rounds of 512 workgroups, 64 x 128 tiles for the rows left (`bands`)
//   Ring        conv_gemm_ring.hip, LDS-DMA ring: a plain (row tiles, column tiles, problems) grid of bm x bn tiles
//   RingDealt   the same tiles dealt to the XCDs in operand-sharing blocks (1-D grid)
//   RingBanded  ring engine: bands (`bands`) + dealt tiles
//   RingSK      ring engine: whole tiles for the whole units of 256 + a stream-K band (`sk`; not bit-identical with the others)
//   Taps48      conv_taps48.hip: batched problems of 48-channel taps
//   Split       conv_gemm_split.hip: the bf16 matrix cores with fp32 operands split into `planes` terms
//   Invalid     no kernel: an unknown tile id
enum class ConvEngine { Reg, RegBanded, Ring, RingDealt, RingBanded, RingSK, Taps48, Split, Invalid };
struct ConvPlan {
    ConvEngine engine = ConvEngine::Invalid;
    int bm = 0, bn = 0, wm = 0, wn = 0, bk = 32;   // Reg / Ring / RingDealt: the tile and one wave's share of it
    int planes = 0;                                // Split
    ConvBands bands{};                             // RegBanded, RingBanded
    ConvSK sk{};                                   // RingSK
};
// Host only, no HIP call: the plan for a layer.  tile: 0 = the production choice under `k`; otherwise a tile id of ts_op_conv1d_timed
// (include/talkshow_hip_debug.h).  sk_hw: the device passed the stream-K band's hardware check (conv_sk_supported).
ConvPlan plan_conv(const ConvParams &p, int tile, const Knobs &k, bool sk_hw);
// Host only, no HIP call: why launch_conv_plan refuses (p, plan) — a layout the plan's kernel does not implement — or null if it launches
const char *conv_plan_refusal(const ConvParams &p, const ConvPlan &plan);
hipError_t launch_conv_plan(const ConvParams &p, const ConvPlan &plan, hipStream_t stream);
hipError_t launch_conv_gemm(const ConvParams &p, int tile, hipStream_t stream);   // = launch_conv_plan(p, plan_conv(p, tile, knobs(), ...))

// conv_gemm_split's XCD-aware tile order (one definition for the kernel and for the host-side test): workgroup `bid` of a 1-D grid of
// 8 ceil(MT NT / 8) -> tile (tx, ty) of an MT x NT tile grid, false if the workgroup has no tile.  Workgroup ids go round-robin over the 8
// XCDs; XCD x takes the x-th contiguous eighth of a tile list that runs through column groups of GW tiles, rows inside a group, columns fastest.
__host__ __device__ inline bool split_tile_of(int bid, int MT, int NT, int GW, int &tx, int &ty) {
    const int total = MT * NT, per = (total + 7) >> 3;
    const int L = (bid & 7) * per + (bid >> 3);
    if (L >= total) return false;
    const int full = NT / GW;
    int g = L / (MT * GW), r = L - g * MT * GW, gn = GW;
    if (g >= full) {   // the last, narrower column group
        g = full;
        r = L - full * MT * GW;
        gn = NT - GW * full;
    }
    tx = r / gn;
    ty = g * GW + (r - tx * gn);
    return true;
}

// Weights of a layer as the plane images conv_gemm_split builds in LDS — per row and chunk of 32 k: 16 dwords of bf16(x) pairs, then 16
// dwords of bf16(x - bf16(x)) pairs; the same size and pitch as the fp32 matrix (rows x K floats, K % 32 == 0).  Done once per layer when
// the x3 plan is selected: weights are constants, only the activations need splitting per call.
hipError_t launch_split_weight_planes(const float *w, float *planes, long rows, int K, hipStream_t stream);
// Host only, no HIP call: why conv_gemm_split.hip cannot run p with `planes` planes as laid out (the 16-byte loads, the K chunk of 32, plane
// images), or null; and the tile edge its launcher takes (128 or 64) with the workgroups of its grid.
const char *conv_split_refusal(const ConvParams &p, int planes);
int conv_split_tile(const ConvParams &p, long *workgroups);
double conv_gemm_flops(const ConvParams &p);

// ------------------------------------------------------------------------------------------------
// Winograd F(4,3) lowering of the wide stride-1 k = 3 C -> C layers (conv_wino.hip has the matrices, the tiling and the summation orders;
// models.cpp::run_stack_n the sequence).  A lowering like the two output phases of a ConvTranspose: decided above plan_conv by the layer's
// own geometry, never by B, T, the pass form or the stream, so a clip's bits do not depend on the batch it rides in.
// ------------------------------------------------------------------------------------------------
constexpr int WINO_MIN_C = 512;   // TS_CONV_WINO=-1: layers at least this wide are lowered (the audio encoder's widest stack, 256, stays direct)
// knob: Knobs::conv_wino (-1 by width, 0 never, 1 every eligible geometry)
inline bool wino_lowered(int kind, int k, int cin, int cout, int knob) {
    const bool geom = kind == 0 && k == 3 && cin == cout && cin % 32 == 0;
    return geom && knob != 0 && (knob == 1 || cout >= WINO_MIN_C);
}
struct WinoParams {
    int nnet;              // 1 or 2 networks (grid y): body + hands in one launch
    int B, L, J, C;        // clips, rows per clip, tiles per clip = ceil(L / 4), channels (% 4 == 0; rows are C floats apart, 16-byte aligned)
    int act;               // ConvParams::act codes
    const int *lens;       // mixed passes: L_b = min(L, (lens[b] >> len_shr) << len_shl); null: L_b = L
    int len_shr, len_shl;
    const float *x[2];     // wino_in: (B, L, C)
    float *V[2];           // wino_in, wino_out_in: (6, B J, C)
    const float *O[2];     // wino_out, wino_out_in: (6, B J, C)
    const float *bias[2];  // [C]
    const float *res[2];   // wino_out, optional: (B, L, C), added before the activation
    float *y[2];           // wino_out: (B, L, C); every row is written, rows in [L_b, L) as zeros
    // wino_codes only: the layer's input rows are rows of a table, one code per row
    const int64_t *codes[2];   // (B, L) code indices; a row outside [0, L_b) is never read, a code outside [0, ncode) is the zero row
    const float *T[2];         // (6, ncode, C): T_i = table U_i^T (models.cpp::ts_vqvae_create)
    int ncode[2];
    float *Ow[2];              // (6, B J, C): what wino_in and the layer's six GEMMs would leave in O
    int deal;                  // set by launch_wino: 0 = grid (blocks, nnet); else blocks per network of a 1-D grid dealt to the XCDs in contiguous runs
};
// which: 0 wino_in (x -> V), 1 wino_out (O -> y), 2 wino_out_in (O of layer k -> V of layer k + 1), 3 wino_codes (codes -> O of the first layer)
hipError_t launch_wino(int which, const WinoParams &p, hipStream_t stream);
// host: the six transformed matrices of folded taps w (cout, cin, 3), computed in double and rounded once; out (6, npad, cin)
void wino_transform_weights(const float *w, int cout, int cin, int npad, float *out);

// ------------------------------------------------------------------------------------------------
// skinny_gemm_f32: out[M x N] = A[M x K] * W[N x K]^T with M = a few tens of rows (the batch of clips at one
// code position).  The A operand is a concatenation of up to 6 segments, each either a dense row-major
// block or rows gathered from a table through an int32 index (token -> embedding row).  Each workgroup owns
// 32 output columns and splits K over its waves; epilogues fuse bias, an additive term, the per-class
// conditioning and the tanh*sigmoid gate.
// ------------------------------------------------------------------------------------------------
struct SkinnySeg {
    const float *base;   // dense: row m at base + (m >> row_shift) * row_stride (+ col offset baked in base); null = zero rows
    const int *gidx;     // gather: row = base + gidx[m * gidx_stride] * row_stride ; negative index -> zero row
    long row_stride;
    long gidx_stride;
    int row_shift;
    int len;             // multiple of 8
    int tiled_w;         // 0 = row-major; else the buffer is TILED with this row width (see SkinnyParams::w_tiled)
};

enum { EPI_LINEAR = 0, EPI_GATE = 1 };
constexpr int SKINNY_MAX_SEG = 3;
constexpr int SKINNY_MAX_PROBLEMS = 6;

struct SkinnyParams {
    int M, N;            // N = number of weight rows (EPI_GATE: 2*gateD per group)
    int nseg, Ktot;
    SkinnySeg seg[SKINNY_MAX_SEG];
    const float *W;      // weight row n at W + n*ldw (K-contiguous, Ktot floats used)
    long ldw;
    const float *bias;   // [N] or null
    const float *add1;   // optional: add1[(m >> add1_shift) * add1_stride + n]
    long add1_stride;
    int add1_shift;
    const float *add2;   // optional second additive term, same indexing scheme
    long add2_stride;
    int add2_shift;
    const float *add3;   // optional third additive term: add3[m * add3_stride + n]
    long add3_stride;
    const float *clsrow; // optional per-row conditioning added AFTER `pre` is stored: clsrow[m * cls_ld + (n % cls_ld)]
    int cls_ld;
    int epi;             // EPI_LINEAR / EPI_GATE
    int relu;            // EPI_LINEAR only
    int gateD;           // EPI_GATE: channels per gate half (columns n and n+gateD pair up inside each 2*gateD group)
    float *out;          // EPI_LINEAR: [M][out_stride] N columns; EPI_GATE: [M][out_stride], N/2 columns
    long out_stride;
    float *pre;          // EPI_GATE optional: pre-activation (acc + bias + add1 + add2, without clsrow) [M][pre_stride]
    long pre_stride;
    int grid_x, grid_y;  // filled by the launcher
    // ---- tiled operand layouts (descriptor kernel only) ----
    // A wave's MFMA operand fragment is 16 rows x 16 k: lane (i = lane & 15, g = lane >> 4) holds k = 16 q + 4 g .. + 3 of row i.
    // Row-major, one wave load touches 16 rows x 64 B — measured at 14 B/clk/CU from a warm L2 against 34-42 B/clk for a
    // contiguous 1 KB (tools/fetch_rate.cpp).  A TILED buffer stores each such fragment contiguously, in lane order:
    //   float index of element (m, k) of a [rows][W] array = (((m >> 4) * (W >> 4) + (k >> 4)) << 8) + (((m & 15) + 16 * ((k & 15) >> 2)) << 2) + (k & 3)
    // rows padded to a multiple of 16, W a power of two >= 16.  Weights: tile t (16 output columns, in the epilogue's
    // column order), q-step q at ((t * (K / 16) + q) << 8), same lane order.
    int w_tiled;         // 0: W is row-major [N][ldw]; else W is the tiled copy and this is K / 16
    int out_tiled_w;     // 0 or the row width of the tiled view `out` is written in (element (row, col) = linear row * out_stride + col)
    int pre_tiled_w;     // same for `pre`
    int add1_tiled_w;    // same for reading `add1`
};

// up to SKINNY_MAX_PROBLEMS INDEPENDENT problems share one launch (blockIdx.z): one kernel boundary on the dependent chain
struct SkinnyBatch {
    SkinnyParams p[SKINNY_MAX_PROBLEMS];
};

// The K split of the 16-column chain kernels (wide, fast, generic 16-column): the waves a launch whose largest problem has depth K runs on.
// The one statement of the rule: plan_skinny, the code tables and pixelcnn.cpp's launch_slot all take it from here.  (The generic
// 32-column kernel, which odd shapes fall to, has its own rule in plan_skinny and is outside the bit contract.)
inline int skinny_waves16(int K) { return K >= 256 ? 8 : 4; }
// host-side: the tiled copy of a weight matrix W [N][ldw] (K columns used) for epilogue `epi` (column order of EPI_GATE tiles:
// 8 "tanh" channels followed by their 8 "sigmoid" partners); out has ceil(N/16) * (K/16) * 256 floats
void skinny_tile_weights(const float *W, int N, int K, long ldw, int epi, int gateD, float *out);
// false if an environment knob forces the generic kernels (which do not read tiled operands)
bool skinny_descriptor_kernel_enabled();
hipError_t launch_skinny_gemm(const SkinnyParams &p, hipStream_t stream);
// Which kernel runs a batch of chain problems (skinny_gemm.hip::plan_skinny): Wide = skinny_wide.hip's 64 x 64 full-K tiles, Fast = the
// descriptor kernel skinny16_fast_kernel<W, RB, CB> (tiles of RB x CB blocks of 16 x 16, K split over W waves), Generic16 / Generic32 = the
// row-major kernels with 16- / 32-column workgroups (W waves); Invalid = the problems fit no kernel.
enum class SkinnyKernel { Wide, Fast, Generic16, Generic32, Invalid };
struct SkinnyPlan {
    SkinnyKernel kernel = SkinnyKernel::Invalid;
    int W = 0, RB = 0, CB = 0;
    int total = 0;                        // Wide / Fast: workgroups of the 1-D grid
    int gx = 0, gy = 0;                   // Generic: the (gx, gy, problems) grid
    int items[SKINNY_MAX_PROBLEMS] = {};  // Wide: tiles per workgroup of each problem
    int start[SKINNY_MAX_PROBLEMS] = {};  // Wide / Fast: first workgroup of each problem
};
// Host only, no HIP call: the plan for n problems under `k`.  Wide and Fast need the descriptors to pack and the zero buffer; where either
// is missing, launch_skinny_batch runs Generic16 with the plan's W.
SkinnyPlan plan_skinny(const SkinnyParams *const *ps, int n, const Knobs &k);
hipError_t launch_skinny_batch(const SkinnyParams *const *ps, int n, hipStream_t stream);   // = the form below under knobs()
// the same launch under the levers `k` (a trace instance only where skinny_init made the record buffer); ran (optional) = the plan that
// actually launched: a Wide or Fast plan whose descriptors did not pack, or without the zero buffer, reports Generic16 with the plan's W
hipError_t launch_skinny_batch(const SkinnyParams *const *ps, int n, hipStream_t stream, const Knobs &k, SkinnyPlan *ran);
// allocates the per-device zero buffer the fast skinny kernel substitutes for absent operands (call once per device,
// outside stream capture; without it the generic kernels are used)
hipError_t skinny_init(int device);
// the per-device zero buffer (256 KB) allocated by skinny_init, or nullptr
const float *skinny_zero_buffer(int device);
// TS_SKINNY_TRACE=1 instrumentation: records of 6 u64 {t_entry, t_desc, t_mfma_done, t_reduced, t_end, cnt<<32|workgroups}
int skinny_trace_read(unsigned long long *out, int max_records);

// ---- code tables of the chain (code_tables.hip): slot V0 and column 1's hg_0 as lookups of slice sums ----
// The K split of a chain GEMM: W waves (plan_skinny's rule for the 16-column kernels), wave w owning q-steps [Q w / W, Q (w + 1) / W) of 16 k
inline int code_table_waves(int K) { return skinny_waves16(K); }
constexpr int CODE_TABLE_MAX_SETS = 5;   // row sets of a table: one prefix (the first code's slices) + one per slice of a second code (W / 2 <= 4)
// one row set: out[code][0..N) = sum in index order of slices [s0, s1) of W[n][k] . emb[code][k - kcol], K = the GEMM's whole K
struct CodeTableBuild {
    const float *W;     // [N][ldw] row-major
    long ldw;
    int N, K, waves, s0, s1;
    const float *emb;   // [V][D]
    int D, V, kcol;
    float *out;         // [V][N]
};
hipError_t launch_code_table_build(const CodeTableBuild &p, hipStream_t stream);
// the gate problem of a slot (+ up to two linear riders that share its codes) from tables; see code_tables.hip for the arithmetic
struct CodeTableStage {
    const float *tab[3];       // gate, rider 0, rider 1: [nsets][V][N]
    long set_stride;           // V * N
    int nsets;                 // 1: only tok0 (prefix rows); 1 + s: tok1's s slice rows are added one by one behind it
    int M, N, gateD;           // clips; channels (weight rows) = groups of gateD tanh + gateD sigmoid
    const int *tok0, *tok1;    // code of clip m at tok[m * tok_stride]; negative: the zero row
    long tok_stride;
    const float *bias, *add1, *add2;   // [N] / (M, stride) rows; null: +0.0
    long add1_stride, add2_stride;
    const float *cls;          // (M, cls_ld) class-conditioning rows, column n % cls_ld
    int cls_ld;
    float *pre;                // pre-gate values (M, pre_stride) or null; pre_tw: log2 of its tiled view width, 0 row-major
    long pre_stride;
    int pre_tw;
    float *out;                // gated values (M, out_stride), N / 2 per clip
    long out_stride;
    int out_tw;
    float *rider[2];           // (M, rider_stride) rows of N, or null
    long rider_stride;
};
hipError_t launch_code_table_stage(const CodeTableStage &p, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// VQ / sampling / glue kernels
// ------------------------------------------------------------------------------------------------
// idx[m] = argmin_j (|x_m|^2 + |e_j|^2) - 2 x_m.e_j   (ties -> lowest j); also writes int32 copy if idx32 != null
hipError_t launch_vq_argmin(const float *x, int ldx, int M, const float *codebook, const float *code_sq, int ncode,
                            int dim, int64_t *idx, long idx_stride, hipStream_t stream);
// The codebook search of a MIXED pass for both networks at once (talkshow_hip.h, "given poses"): row m = b * H + h of network n is valid iff
// h < lens[b] >> 2 (lens: device table of pose frame counts, any order).  codes[(b * Hout + h) * 2 + n] = the index launch_vq_argmin returns
// for that row if it is valid, -1 if not (the row of z is then never read).  z[n] (B * H, dim[n]) contiguous rows.
struct VqPairParams {
    const float *z[2], *cb[2], *csq[2];
    int ncode[2], dim[2];
    int B, H, Hout;      // Hout >= H: rows per clip of the code block (rows h >= H of it are left alone)
    const int *lens;
    int64_t *codes;
};
// form 0: the library's choice (one paired LDS launch where both networks have dim = 64 and one ncode; TS_VQ_PAIR=0: two launches of it);
// 1 / 2: paired / two launches named outright (tools, tests); 3: two launches of the masked generic kernel, which is also where every
// configuration the LDS form does not cover goes
hipError_t launch_vq_argmin_pair_masked(const VqPairParams &p, int form, hipStream_t stream);
// code_sq[j] = sum_c e[j][c]^2
hipError_t launch_row_sqnorm(const float *e, int n, int dim, float *out, hipStream_t stream);
// out[m][0..width) = table[idx[m*idx_stride]][0..width); an index outside [0, nrows) gives a row of NaNs
hipError_t launch_gather_rows(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M,
                              int width, float *out, int ldo, hipStream_t stream);
// the same for a padded batch of clips (mixed passes): row m = b * L + t with t >= lens[b] >> len_shr is written as a ZERO row whatever
// idx holds there (the index is not read); rows inside the clip keep the NaN answer to a bad index
hipError_t launch_gather_rows_masked(const float *table, int ld_table, int nrows, const int64_t *idx, long idx_stride, int M,
                                     int width, float *out, int ldo, int L, const int *lens, int len_shr, hipStream_t stream);
// speaker style (talkshow_hip.h): out[l][rr][slot][0..W) for the rows [r0, r0 + n) of `slots` clip slots and NL layers, from float weights
// (slots, S, NC) with rows w_ld floats apart (S == 1: one row per slot for every code row) and the NL class tables [NL][NC][W]:
// the ascending sum of w[c] * E_l[c] over the non-zero weights, product and sum rounded separately, +0.0 if there is none.
// lens (optional, (slots,)): rows at or beyond lens[slot] >> len_shr take the weights of the slot's last own row.
struct StyleRowsParams {
    const float *tables;
    const float *weights;
    long w_ld;
    int S, NC, W, NL;
    int r0, n, slots;
    const int *lens;
    int len_shr;
    float *out;
    long out_l_stride, out_r_stride;   // floats between the layers / the rows of `out`; slots are W apart
};
hipError_t launch_style_rows(const StyleRowsParams &p, hipStream_t stream);
// dst[b][t][0..cpad) = src[b][t][0..c) then zeros for t < lens[b], a zero row for t >= lens[b]  (B clips of L rows)
hipError_t launch_pad_rows_masked(const float *src, int lds, int c, float *dst, int ldd, int cpad, int B, int L, const int *lens,
                                  hipStream_t stream);
// codes[b][r][0..1] = -1 for r >= lens[b] >> 2  (B clips of H rows of 2 codes: the documented padding of a mixed pass)
hipError_t launch_mask_codes(int64_t *codes, int B, int H, const int *lens, hipStream_t stream);
// dst[b] = first + b (the per-clip Philox subsequences of a mixed pass that was given no table)
hipError_t launch_iota_i64(int64_t *dst, int n, int64_t first, hipStream_t stream);
// dst[m][0..cpad) = src[m][0..c) then zeros
hipError_t launch_pad_rows(const float *src, int lds, int c, float *dst, int ldd, int cpad, long M, hipStream_t stream);
// (B,Tb,129) body/hand poses + (B,Tf,103) jaw/expression -> (B,Tf,265) full SMPL-X parameter rows (demo.py:207-229, part2full)
hipError_t launch_assemble_full(const float *body, const float *face, const float *lower_pose33, int B, int Tb, int Tf,
                                float *out, hipStream_t stream);
// the same for a padded batch (mixed passes): tb / tf = device tables of the clips' own body and face frame counts; rows t < tf[b] as above on
// the clip alone (body frame min(t, tb[b] - 1)), rows t >= tf[b] written as 0
hipError_t launch_assemble_full_lens(const float *body, const int *tb, const float *face, const int *tf, const float *lower_pose33, int B,
                                     int Tb, int Tf, float *out, hipStream_t stream);
// int64 -> int32 (labels, teacher-forced codes)
hipError_t launch_i64_to_i32(const int64_t *src, int *dst, long n, hipStream_t stream);
// test aid: out[i] = gate_act(v[i], p[i])
hipError_t launch_gate_act(const float *v, const float *p, float *out, long n, hipStream_t stream);
// test aid: out[i] = gelu_fast(v[i])
hipError_t launch_gelu(const float *v, float *out, long n, hipStream_t stream);
// dst[0..2] = a, b, c, carried by the launch's own arguments (no host buffer has to outlive the call)
hipError_t launch_set_words3(uint64_t *dst, uint64_t a, uint64_t b, uint64_t c, hipStream_t stream);
// measurement aid: n records of (wall ticks since start, wall ticks of the window, shader cycles of the window), 100 MHz wall clock
hipError_t launch_clock_sample(unsigned long long *out, int n, unsigned long long window_ticks, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// Test / A-B levers (INTEGRATION.md has the table).  Every TS_* environment variable the library knows is read ONCE, by the
// first ts_ctx_create of the process (api.cpp), into this struct; nothing on a launch path calls getenv.  All paths behind
// them are bit-identical on a clip's codes (tests/test_gpu_parity.py::test_alternate_kernel_paths).
// ------------------------------------------------------------------------------------------------
struct Knobs {
    bool conv_bands = true;     // TS_CONV_BANDS=0: big conv layers as one plain grid of 128 x 128 tiles
    bool vq_lds = true;         // TS_VQ_LDS=0: the codebook search reads code rows from L2 per thread instead of LDS-staged tiles (tests, A/B)
    bool vq_pair = true;        // TS_VQ_PAIR=0: the mixed pass's codebook search as two launches (one per network) instead of one paired launch; same indices (A/B, tools/poses_pass.py)
    int conv_ring = 9;          // TS_CONV_RING=0|1|3|8|9: single-problem layers that take 128 x 128 tiles on conv_gemm.hip (0) / forced onto the ring engine's 128 x 128 tile with 4 (1) or 8 (8) waves or its 96 x 128 tile (3) / (9, default) 128 x 128 on 8 waves or 96 x 128 by tile count
    bool w2v_moments = true;    // TS_W2V_MOMENTS=0: conv0's GroupNorm statistics from a pass that computes the convolution (512 channels) instead of from the input's second moments (A/B, tests)
    int conv_sk = 1;            // TS_CONV_SK=0: no stream-K band in the ring engine's plans (whole tiles only: the round-5 plans); 2: the band wherever a layer has a plan for one (A/B, tests)
    bool face_pack = false;     // TS_FACE_PACK=1: mixed face passes on the packed plan — feature convolutions and transformer rows over the clips' own rows back to back instead of B x longest; same bits; off until padded and packed have been timed side by side
    bool conv_taps48 = true;    // TS_CONV_TAPS48=0: the face generator's grouped positional conv as 64-channel windows on conv_gemm_f32's tiles instead of conv_taps48.hip (A/B, tests)
    bool conv_ring_paired = true;    // TS_CONV_RING_PAIRED=0: paired layers (two problems per launch: body + hands) on conv_gemm.hip's banded launch instead of the ring engine (A/B, tests)
    bool conv_deal = true;      // TS_CONV_DEAL=0: the ring engine's tiles as a plain (row tiles, column tiles) grid instead of dealt to the XCDs in operand-sharing blocks (A/B, tests)
    int split_xcd = 8;          // TS_SPLIT_XCD: column-group width of conv_gemm_split's XCD-aware tile order (0: plain 2-D tile grid)
    bool prof_log = false;      // TS_PROF_LOG=1: one stderr line per conv launch while ts_prof is enabled
    bool no_graph = false;      // TS_NO_GRAPH=1: PixelCNN launches go out eagerly
    int pix_defer_p = -1;       // TS_PIX_DEFER_P: -1 auto (<= 128 clips), 0 / 1 forced
    int pix_tables = -1;        // TS_PIX_TABLES: slot V0 and column 1's hg_0 from code tables (code_tables.hip): -1 auto (passes of >= 64 clips), 0 never (the GEMM launches; no tables are built), 1 every pass
    int skinny_v = 1;           // TS_SKINNY_V=0: generic chain kernels
    int skinny_nt = 16;         // TS_SKINNY_NT=32: 32-column generic kernel
    bool skinny_tiled = true;   // TS_SKINNY_TILED=0: row-major chain operands
    int wide_min = 160;         // TS_SKINNY_WIDE_MIN: workgroups from which a coalesced launch takes the wide kernel (0 never, 1 always)
    int skinny_shape = 0;       // TS_SKINNY_SHAPE=11|21|22|42: forced split-K tile shape
    int skinny_trace = 0;       // TS_SKINNY_TRACE=1: in-kernel clock stamps (tools/skinny_trace.py, tools/wide_trace.py)
    bool wide_pair = true;      // TS_SKINNY_WIDE_PAIR=0: the wide kernel's tiles enumerated column-major instead of (clip-block pair, column tile, block of the pair) (A/B, tests)
    int wide_ablate = 0;        // TS_SKINNY_WIDE_ABLATE=2|4 (trace builds): no loads / no MFMAs in the wide kernel
    int conv_wino = -1;         // TS_CONV_WINO: the Winograd F(4,3) lowering of stride-1 k = 3 C -> C layers: -1 from WINO_MIN_C channels on, 0 never (direct everywhere), 1 every eligible geometry (tests).  Read when a network is created
    bool wino_deal = true;      // TS_WINO_DEAL=0: the Winograd transform kernels on a plain (blocks, networks) grid instead of dealt to the XCDs in contiguous runs (A/B, tests; the same bits)
    int vq_dec_tables = -1;     // TS_VQ_DEC_TABLES: the VQ decoders' first Winograd-lowered layer from per-code tables (conv_wino.hip::wino_codes): -1 where that layer is lowered and the network has a codebook, 0 never.  Read when a network is created
};
const Knobs &knobs();

// ---- code tables: host arithmetic (ts_debug_code_tables_plan, tests/test_code_tables_host.py) ----
// Tables are skipped, and the GEMM launches kept, where V x 4D x 4 B x 15 (the three V0 tables at five row sets) exceeds this: the
// shipped network (V = 2048, D = 256) takes 120 MiB + 4 MiB, an odd configuration still loads
constexpr size_t CODE_TABLE_CAP_BYTES = (size_t)192 << 20;
// TS_PIX_TABLES = -1: passes (chunks of a mixed pass: their active clips) of at least this many clips take the tables.  Bits are equal
// either way, so the rule is free; the measurement behind it is in DESIGN.md §4
constexpr int CODE_TABLE_MIN_CLIPS = 64;
struct CodeTablePlan {
    bool fits = false;                   // under the cap, and on kernels whose K split the tables reproduce (not TS_SKINNY_NT=32)
    int waves_v0 = 0, sets_v0 = 0, waves_hg = 0;
    size_t bytes_v0 = 0, bytes_hg = 0;   // all three V0 tables; the hg_0 table
};
inline CodeTablePlan code_table_plan(int V, int D, const Knobs &k) {
    CodeTablePlan t;
    if (V < 1 || D < 32 || D % 32) return t;
    t.waves_v0 = code_table_waves(2 * D);
    t.sets_v0 = 1 + t.waves_v0 / 2;
    t.waves_hg = code_table_waves(D);
    t.bytes_v0 = (size_t)3 * t.sets_v0 * V * 4 * D * sizeof(float);
    t.bytes_hg = (size_t)V * 2 * D * sizeof(float);
    t.fits = k.skinny_nt != 32 && (size_t)V * 4 * D * sizeof(float) * 15 <= CODE_TABLE_CAP_BYTES;
    return t;
}
inline bool code_table_pass(bool built, int mode, int B) { return built && (mode > 0 || (mode < 0 && B >= CODE_TABLE_MIN_CLIPS)); }
// which launches of code row r become lookups: slot V0 from row 1 on (row 0 has no code above it), hg_0 of column 1 only (column 0 has
// none to its left); a rider is written iff the row it serves is generated (the GEMM riders' rule)
inline bool code_table_v0_row(int r) { return r >= 1; }
inline bool code_table_hg_col(int j) { return j == 1; }
inline bool code_table_rider(int r, int t, int last_row) { return r >= 1 && r + (2 - t) < last_row; }   // t = 1: Q1 of row r+1, t = 0: Q0 of row r+2


// GELU(x) = x / 2 (1 + erf(x / sqrt 2)) for the conv epilogues of the face generator (reference: torch's exact-erf GELU behind the HF wav2vec2
// layers of nets/spg/wav2vec.py).  libm's erff is two branches (|x| < 1: an odd polynomial; else 1 - exp(-poly)) with expf's own range
// reduction: ~45 VALU instructions plus exec-mask juggling per element, and on the ring engine's 8-wave tiles it is NOT hidden — measured
// (tools/gelu_cost.py): +42 us on a 692 us FFN1, +92 us on a 1.04 ms feature-convolution shape.  Here both pieces of the same algorithm with
// the same coefficients run branch-free (v_cndmask) and the exponential is one v_exp_f32: ~22 instructions, |error| <= 9e-8 (1 ulp of erf)
// against float64 over [-6, 6] — the face's distance from the reference does not move (2e-6).
__device__ __forceinline__ float erf_fast(float x) {
    const float a = __builtin_fabsf(x), t = a * a;
    float p = __builtin_fmaf(t, -0.000561801774892956f, 0.004913816228508949f);
    p = __builtin_fmaf(t, p, -0.026707515120506287f);
    p = __builtin_fmaf(t, p, 0.11280010640621185f);
    p = __builtin_fmaf(t, p, -0.37612295150756836f);
    p = __builtin_fmaf(t, p, 0.12837910652160645f);
    const float r1 = __builtin_fmaf(a, p, a);                       // |x| < 1
    float q = __builtin_fmaf(a, 1.699881067906972e-05f, -0.00037867785431444645f);
    q = __builtin_fmaf(a, q, 0.003857815871015191f);
    q = __builtin_fmaf(a, q, -0.024181697517633438f);
    q = __builtin_fmaf(a, q, 0.10666826367378235f);
    q = __builtin_fmaf(a, q, 0.6349332928657532f);
    q = __builtin_fmaf(a, q, 0.12868940830230713f);
    q = __builtin_fmaf(a, q, a);
    const float r2 = 1.0f - __builtin_amdgcn_exp2f(-1.4426950408889634f * q);   // |x| >= 1; exp2 of a large negative number flushes to 0
    return __builtin_copysignf(a < 1.0f ? r1 : r2, x);
}
__device__ __forceinline__ float gelu_fast(float v) { return 0.5f * v * (1.0f + erf_fast(v * 0.70710678118654752440f)); }

// tanh(v) * sigmoid(p) of GatedActivation (gated_pixelcnn_v2.py:16-22) on the hardware exponential and reciprocal (v_exp_f32,
// v_rcp_f32: 1 ulp each): tanh(v) = 1 - 2 / (1 + e^(2v)), sigmoid(p) = 1 / (1 + e^(-p)) — 10 instructions per gate value where
// tanhf + expf + a division took ~45 (8 values per lane in the wide kernel's epilogue: half of its VALU instructions, on the
// dependent chain of 30 launches per code row).  Absolute error < 2e-7 (the gate is O(1)); saturates correctly (e^(2v) = inf -> 1,
// flushed to 0 -> -1).  The RELATIVE error of the tanh factor grows towards v = 0 (1 - 2 / (1 + e^(2v)) cancels: ~6e-8 / |v|), which
// is harmless where the value is used — it is added into O(1) sums by the next layer — and is measured, absolute and relative, by
// tests/test_gpu_parity.py::test_gate_activation_accuracy over the whole input range (ts_debug_gate_act).
// ONE definition for every chain kernel: a clip's bits must not depend on which kernel served its stage.
__device__ __forceinline__ float gate_act(float v, float p) {
    const float ev = __builtin_amdgcn_exp2f(v * 2.88539008177792681f);      // e^(2 v)
    const float ep = __builtin_amdgcn_exp2f(p * -1.44269504088896341f);     // e^(-p)
    const float th = fmaf(-2.0f, __builtin_amdgcn_rcpf(1.0f + ev), 1.0f);
    return th * __builtin_amdgcn_rcpf(1.0f + ep);
}

// exp(x) for x <= 0 from fp32 multiplies and adds ONLY (no fused multiply-add, no hardware transcendental): every operation is
// one IEEE round-to-nearest fp32 operation, so `oracle/talkshow_oracle.py::det_expf` reproduces it bit for bit on any host and
// the inverse-CDF draw of a given uniform is the same index on the device and in the oracle — not "within one slot".
// Cody-Waite reduction by ln 2 (n * LN2_HI is exact), degree-5 polynomial on [-ln2/2, ln2/2] (Cephes' coefficients), 2^n by
// exponent bits; relative error < 2 ulp.  Arguments below -86 give 0 (2^-124: everything stays a normal number).
__device__ inline float det_expf(float x) {
#pragma clang fp contract(off)
    if (x < -86.0f) return 0.0f;
    const float n = rintf(x * 1.44269504088896341f);
    float r = x - n * 0.693145751953125f;
    r = r - n * 1.42860682030941723212e-6f;
    float q = 1.9875691500e-4f;
    q = q * r + 1.3981999507e-3f;
    q = q * r + 8.3334519073e-3f;
    q = q * r + 4.1665795894e-2f;
    q = q * r + 1.6666665459e-1f;
    q = q * r + 5.0000001201e-1f;
    float y = q * (r * r) + r;
    y = y + 1.0f;
    return y * __int_as_float(((int)n + 127) << 23);
}

struct SampleParams {
    const float *logits;   // row b at logits + b * (logit_stride ? logit_stride : V)
    long logit_stride;     // 0 = V (contiguous rows)
    int B, V;
    int mode;              // TS_SAMPLE_* ; TEACHER_FORCED copies
    const float *uniforms; // element for clip b at uniforms[b * u_stride]
    long u_stride;
    uint64_t seed;
    int64_t clip_index0;
    const uint64_t *dyn;   // optional device words {seed, clip_index0, position base}: the first two override the fields above, the
                           // third is added to `position` (graph replay: a captured chunk serves every chunk of a session)
    uint32_t position;     // Philox counter word: linear position (row*2 + col)
    int *tok32;            // token for clip b written to tok32[b * tok_stride]
    long tok_stride;
    int64_t *codes;        // same position in the int64 output, codes[b * code_stride]
    long code_stride;
    float *logits_copy;    // optional: logits_copy[b * copy_stride + v] = logits[b][v]
    long copy_stride;
    const int64_t *clip_table;   // optional: clip b draws from Philox subsequence clip_table[b] instead of clip_index0 + b (mixed passes)
    const int32_t *row_origin;   // optional ("slot restart", talkshow_hip.h): clip b's Philox counter word is the position minus 2 * row_origin[b],
                                 // the position inside the slot's CURRENT clip; everything else (given bounds, history rings) stays in session rows
};
hipError_t launch_sample(const SampleParams &p, hipStream_t stream);

// "slot restart" of a streaming session (talkshow_hip.h): for each of the n listed clip slots, write "nothing above row `row`" into the row
// cache — the slots' entries of the token ring rows row-1 .. row-3 (those >= 0) become -1 (a negative gather index is the zero row), their
// rows of Q1[row & 3], Q0[row & 3] and Q0[(row + 1) & 3] become +0.0, their row of P(l, row & 1) becomes bv[l] for l >= 1 — and, from labels,
// their conditioning rows CR[l] = tables[l][label] (a copy: the label's bits); row_origin[slot] = row.  Those rows of those slots and nothing
// else.  Every buffer is row-major with slabs of B clips; slots / labels are device tables the host wrote in stream order.
struct SlotResetParams {
    const int32_t *slots;    // (n,) in [0, B)
    const int32_t *labels;   // (n,) in [0, NC), or null: CR is left to the caller (style rows)
    int n, B, row;
    int D, NL, NC, R;        // R: rows of the token ring tok32[B][R][2]
    int *tok32;
    float *Q1, *Q0;          // [4][B][4D]
    float *P;                // [NL][2][B][4D]
    float *CR;               // [NL][B][2D]
    const float *bv;         // [NL][4D]
    const float *tables;     // [NL][NC][2D]
    int32_t *row_origin;     // (B,)
};
hipError_t launch_slot_reset(const SlotResetParams &p, hipStream_t stream);

// "slot state" of a streaming session (talkshow_hip.h): what a restart writes, read out of one slot and written back at another slot, another
// session row and another buffer phase.  A state is ONE ROW of 32-bit words per slot; the layout is a function of (D, NL) alone (offsets
// in words; every float block starts at a multiple of 4 words, the integer tail is a multiple of 4 words long):
//   q1   [4D]          Q1[r & 3]                      q0a [4D]  Q0[r & 3]             q0b [4D]  Q0[(r + 1) & 3]
//   p    [NL-1][4D]    P(l, r & 1), l = 1 .. NL-1     cr  [NL][2D]  CR[l]
//   tok  [8]  int32    the codes of rows r-1, r-2, r-3 (two columns each: word 2 k + c is row r-1-k, column c), then two words of 0
//   rep  [2][64] int32 the repetition histories BY AGE: word 64 c + k is column c's code of row r-1-k for k < hist, -1 beyond
struct SlotStateLayout {
    int q1, q0a, q0b, p, cr, tok, rep, words;
};
constexpr int SLOT_STATE_TOK_WORDS = 8;
__host__ __device__ inline SlotStateLayout slot_state_layout(int D, int NL) {
    SlotStateLayout L;
    L.q1 = 0, L.q0a = 4 * D, L.q0b = 8 * D, L.p = 12 * D;
    L.cr = L.p + (NL - 1) * 4 * D;
    L.tok = L.cr + NL * 2 * D;
    L.rep = L.tok + SLOT_STATE_TOK_WORDS;
    L.words = L.rep + 2 * 64;
    return L;
}
// Save: state row i = the state of slot slots[i] at session row `row` (the session's NEXT row), canonical for row < 3: an entry the
// session's launches of rows `row` and `row + 1` would not read is saved as the value a restart writes there (token rows below 0 as -1, Q1
// and Q0[(row + 1) & 3] as +0.0 for row < 2, Q0[row & 3] as +0.0 for row < 3, P as bv[l] at row 0).  hist[i]: how many entries of the slot's
// histories mean anything (<= 64; <= 0: none).  open_labels (with tables, NC) set: CR has not been written yet (a session at row 0) and
// the rows are tables[l][open_labels[slot]], what the first step will write.  Reads the session's buffers, writes n rows of `state` only.
struct SlotSaveParams {
    const int32_t *slots;    // (n,) in [0, B); a slot outside writes nothing
    const int32_t *hist;     // (n,)
    int n, B, row;
    int D, NL, NC, R;
    const int *tok32;
    const float *Q1, *Q0, *P, *CR, *bv;
    const int32_t *rep_ring;       // [B][2][64]
    const int64_t *open_labels;    // (B,) or null
    const float *tables;           // [NL][NC][2D], read with open_labels only
    float *state;                  // (n, words)
};
hipError_t launch_slot_save(const SlotSaveParams &p, hipStream_t stream);
// Load: slot slots[i] takes state row index[i] (one row may serve many slots) at session row `row`: the ring rows row-1 .. row-3 that exist,
// Q1[row & 3], Q0[row & 3], Q0[(row + 1) & 3], P(l, row & 1), CR[l], the histories at ring[(row - 1 - k) & 63], row_origin[slot] = origin[i].
// A slot outside [0, B) or an index outside [0, n_states) writes nothing.
struct SlotLoadParams {
    const int32_t *slots, *index, *origin;   // (n,) each
    int n, n_states, B, row;
    int D, NL, R;
    int *tok32;
    float *Q1, *Q0, *P, *CR;
    int32_t *rep_ring;
    int32_t *row_origin;     // (B,)
    const float *state;      // (n_states, words)
};
hipError_t launch_slot_load(const SlotLoadParams &p, hipStream_t stream);

// Per-clip sampling controls (talkshow_hip.h: ts_sampling and the rule of steps 1-5).  The device record of a clip: 1 / temperature as the
// HOST computed it in fp32, top_p, top_k (0 or >= V: off).  A sibling of SampleParams: the sampler without controls keeps its arguments (vq.hip: sample_ctl_body behind
// sample_ctl_kernel<FAST, LP>; the samplers without controls share sample_plain_body).
struct SampleCtl {
    float inv_t, top_p;
    int32_t top_k, pad;
};
// The device record of a clip's repetition penalty: ts_repeat's first three words (window in [0, SAMPLE_REP_RING], 0 = off) and from_row, the
// first absolute row of the clip's current unbroken run of rows written under window > 0: a launch at row r counts min(r - from_row, window)
// ring entries.  0 for every one-shot pass (rep_table): its history starts at row 0.  A streaming session sets it to the row at which a
// clip's penalty was switched on, so that ring entries of rows from before that row are never read
struct SampleRep {
    int32_t window;
    float presence, frequency;
    int32_t from_row;
};
constexpr int SAMPLE_REP_RING = 64;
struct SampleCtlParams {
    SampleParams s;            // mode TS_SAMPLE_UNIFORMS or TS_SAMPLE_PHILOX
    const SampleCtl *ctl;      // record of clip b at ctl[b]
    unsigned char *kept;       // optional (B,V): 1 for the tokens the filters kept
    float *logprob;            // optional: the log-probability of the drawn code (talkshow_hip.h, "log-probabilities") at logprob[b * lp_stride]
    long lp_stride;
    // "code bias" (talkshow_hip.h): bias (NB,2,V) fp32 tables, bias_index[b] the table of clip slot b or -1 (the clip has none and executes
    // the arithmetic of a launch without tables), bias_col 0 (body) / 1 (hand): the row added to the logits ahead of step 1.  Read by the
    // sample_ctl_bias kernels only; null for every other launch
    const float *bias;
    const int32_t *bias_index;
    int bias_col;
    // "repetition penalty" (talkshow_hip.h): rep[b] the record of clip slot b, rep_ring[b][bias_col][64] the codes the slot produced in this
    // column, row r at index r & 63 (r = the launch's absolute position >> 1).  A slot with window 0 reads and writes no ring and executes
    // the arithmetic of the sample_ctl_bias kernels.  Read by the sample_ctl_rep kernels only, which also need bias_index (all -1 and
    // bias null: a pass without tables); null for every other launch
    const SampleRep *rep;
    int32_t *rep_ring;
    // "guidance" (talkshow_hip.h): guide_role[b] the role of clip slot b — -1 plain, g >= 0 a primary whose shadow is slot g, -2 a shadow,
    // whose workgroup returns at once — and guide_scale[b] the scale of a primary.  A primary reads the logits row of slot g through the
    // strides of its own and writes what it chose or was given to both slots' entries of tok32, codes, kept and logprob.  Read by the
    // sample_ctl_guide kernels only, which also need rep, rep_ring and bias_index (records of window 0 / an index of -1: a pass without
    // those pieces); null for every other launch
    const int32_t *guide_role;
    const float *guide_scale;
};
// a histogram bin of the kernel holds count << 44 | mass with mass <= V * 2^31: V * 2^31 < 2^44 bounds the vocabulary (the tie counters' 16 bits
// and the count field hold more); launch_sample_ctl and the host checks refuse anything above
constexpr int SAMPLE_CTL_MAX_V = 8191;
hipError_t launch_sample_ctl(const SampleCtlParams &p, hipStream_t stream);

// The sampler without controls plus the log-probability of the chosen (greedy, drawn) or given (teacher forced: s.codes is read) code:
// logprob[b * lp_stride] = (float)((double)(l_c - max) - log((double)S)), S the sampler's own fp32 total (talkshow_hip.h).  A sibling of
// SampleParams again: sample_kernel keeps its arguments.  vq.hip: sample_lp_kernel = sample_plain_body<LP = true, GIVEN = false>,
// sample_kernel = the same body with both flags off.
struct SampleLpParams {
    SampleParams s;            // any mode
    float *logprob;
    long lp_stride;
};
hipError_t launch_sample_lp(const SampleLpParams &p, hipStream_t stream);
// The three samplers with GIVEN rows (talkshow_hip.h, "given rows"; vq.hip: sample_given_kernel, sample_lp_given_kernel,
// sample_ctl_given_kernel): clip slot b is forced — its code is read from `given`, nothing is drawn — iff the launch's absolute position
// (c.s.position plus the dynamic base word) is below 2 * rows[b].  c: the sibling's arguments (c.s.mode greedy / uniforms / Philox; c.ctl,
// c.kept and c.logprob optional, a table needs a drawing mode).  A sibling of the three structs above again: they keep their arguments.
// The given kernels are the GIVEN = true instantiations of the two bodies their siblings are made of.
struct SampleGivenParams {
    SampleCtlParams c;
    const int *rows;           // (slots,) G of every clip slot of the pass
    const int64_t *given;      // the given code of clip b at given[b * given_stride]; read by forced workgroups only
    long given_stride;
    // "kept positions": the mask byte of clip b at keep[b * keep_stride], read by workgroups below 2 * rows[b] only; a byte of 0 makes the
    // workgroup unforced.  nullptr: every given position is kept, and the kernels execute what they executed before the mask existed
    const unsigned char *keep;
    long keep_stride;
};
hipError_t launch_sample_given(const SampleGivenParams &p, hipStream_t stream);
// "alternatives" (talkshow_hip.h; vq.hip: sample_ctl_alt_kernel, sample_ctl_alt_given_kernel): the launch of the most general unguided
// family — g.c.ctl, g.c.logprob, g.c.bias_index, g.c.rep and g.c.rep_ring are all required (neutral records, an index of -1, records of
// window 0 where the caller brought none); g.rows == nullptr: no given rows — which also writes, for the row of clip b at element e =
// b * stride: codes[e * n + j] / logprob[e * n + j] (j < n; null for n = 0), entropy[e], rank[e].  A sibling of the structs above again:
// they keep their arguments.
constexpr int SAMPLE_ALT_MAX = 8;
struct SampleAltParams {
    SampleGivenParams g;
    int n;                     // 0 .. SAMPLE_ALT_MAX
    int32_t *codes;
    float *logprob;
    float *entropy;
    int32_t *rank;
    long stride;
};
hipError_t launch_sample_alt(const SampleAltParams &p, hipStream_t stream);
// alternatives of a mixed pass: rows at or beyond a clip's own H_b = lens[b] >> 2 hold -1, 0, 0, -1 (codes, log-probabilities, entropy, rank)
hipError_t launch_mask_alt(int32_t *codes, float *logprob, float *entropy, int32_t *rank, int n, int B, int H, const int *lens, hipStream_t stream);
// logprob (B,H,2) rows at or beyond a clip's own H_b = lens[b] >> 2 become 0 (mixed passes; beside launch_mask_codes)
hipError_t launch_mask_logprob(float *logprob, int B, int H, const int *lens, hipStream_t stream);
// Per-clip fixed-order fp64 sums of logprob (B,H,2): out[b] = {body column, hand column, body + hand} over rows r < H_b (lens == nullptr:
// H_b = H, else min(H, lens[b] >> 2)).  Two stages: part[b][t] = the sums of rows t, t + 256, ... in ascending order (t < 256), then the 256
// partials added in ascending order.  scratch: B * 256 * 2 doubles.
constexpr int LOGPROB_SUM_LANES = 256;
hipError_t launch_logprob_sums(const float *logprob, int B, int H, const int *lens, double *scratch, double *out, hipStream_t stream);

// ------------------------------------------------------------------------------------------------
// face generator kernels (face.hip)
// ------------------------------------------------------------------------------------------------
// moments: the GroupNorm statistics from the waveform's second moments (true; production: knobs().w2v_moments) or from a pass that
// computes the convolution (false).  part: B x ceil(L0 / 128) x C double2 of scratch, stats: B x C float2
hipError_t launch_w2v_conv0(const float *wav, int B, int N, int L0, const float *w, const float *gamma, const float *beta,
                            double2 *part, float2 *stats, float *out, int C, bool moments, hipStream_t s);
hipError_t launch_layernorm_rows(const float *x, int ldx, long M, int C, const float *gamma, const float *beta,
                                 const float *post_res, int ldr, int relu, float *out, int ldo, hipStream_t s);
hipError_t launch_lerp_ln(const float *x, int B, int Lin, int T, const float *gamma, const float *beta, float *out,
                          hipStream_t s);
hipError_t launch_attention(const float *qkv, int B, int T, int HID, int heads, float scale, float *out, hipStream_t s);
hipError_t launch_fill_id(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0,
                          int B, int T, hipStream_t s);

// ---- length variants of the same kernels (mixed face passes: B clips of different lengths, padded to N samples / T frames each; `ns` and
// `frames` / `lens` are DEVICE tables of the clips' own sample and frame counts).  A clip's valid rows are the arithmetic of the kernels above
// on the clip alone; rows at or beyond its length are written as zeros (the operand a k = 3 / k = 128 convolution of a clip run alone reads
// past its end) and samples / rows beyond a clip's length are never read ----
// rows of the feature extractor's output for n samples (conv0 k10 s5, then k = 3 3 3 3 2 2 at stride 2, no padding); >= 1 from 400 samples on
__host__ __device__ inline int w2v_feature_rows(int n) {
    int L = (n - 10) / 5 + 1;
    L = (L - 3) / 2 + 1, L = (L - 3) / 2 + 1, L = (L - 3) / 2 + 1, L = (L - 3) / 2 + 1;
    L = (L - 2) / 2 + 1, L = (L - 2) / 2 + 1;
    return L;
}
hipError_t launch_w2v_conv0_lens(const float *wav, int B, int N, const int *ns, const float *w, const float *gamma, const float *beta,
                                 double2 *part, float2 *stats, float *out, int C, bool moments, hipStream_t s);
hipError_t launch_layernorm_rows_lens(const float *x, int ldx, int B, int T, const int *lens, int C, const float *gamma, const float *beta,
                                      const float *post_res, int ldr, int relu, float *out, int ldo, hipStream_t s);
hipError_t launch_lerp_ln_lens(const float *x, int B, int Lin, int T, const int *ns, const int *frames, const float *gamma, const float *beta,
                               float *out, hipStream_t s);
// work: n_work device words, (clip * heads + head) << 10 | query tile or -1 (face.cpp::face_mixed_grid); T <= 65536
hipError_t launch_attention_mixed(const float *qkv, int T, int HID, int heads, const int *work, int n_work, const int *frames, float scale,
                                  float *out, hipStream_t s);
hipError_t launch_fill_id_lens(const float *id, int nc, const float *w, const float *bias, int nj, float *x, int ld, int col0,
                               int B, int T, const int *lens, hipStream_t s);
// ---- packed mixed passes (face.cpp::face_packed_layout): the clips' own rows back to back instead of padded to the longest.  Feature rows:
// clip b owns rows [off[b], off[b + 1]) of ONE time axis at the conv0 rate, off a multiple of 64 (so off[b] >> i is the clip's first row at
// level i of the stride-2 chain); transformer rows: clip b owns rows [row0[b], row0[b] + frames[b]).  off / row0: DEVICE tables of B + 1 words,
// ascending from 0 to the total.  A clip's valid rows are the bits of the length variants above ----
// conv0 with the statistics kernels of launch_w2v_conv0_lens (per clip, same scratch) and the apply pass into out (feat_rows, C): rows
// [off[b], off[b] + L0(ns[b])) = the clip's, zeros up to off[b + 1]; one block per 64 rows of the axis, none for rows no clip has
hipError_t launch_w2v_conv0_packed(const float *wav, int B, int N, const int *ns, const int *off, int feat_rows, const float *w,
                                   const float *gamma, const float *beta, double2 *part, float2 *stats, float *out, int C, bool moments,
                                   hipStream_t s);
// x = level 6 of the packed chain (clip b's rows from off[b] >> 6) -> out (B, T, 512) padded, exactly as launch_lerp_ln_lens writes it
hipError_t launch_lerp_ln_packed(const float *x, int B, int T, const int *ns, const int *frames, const int *off, const float *gamma,
                                 const float *beta, float *out, hipStream_t s);
// dst (rows, C) row row0[b] + t = src (B, T, C) row (b, t) for t < frames[b] = row0[b + 1] - row0[b]; C % 4 == 0
hipError_t launch_pack_rows(const float *src, int B, int T, int C, const int *row0, int rows, float *dst, hipStream_t s);
// dst (B, T, C) row (b, t) = src row row0[b] + t for t < frames[b], +0.0 at and beyond; every element of dst is written
hipError_t launch_unpack_rows(const float *src, const int *row0, const int *frames, int B, int T, int C, float *dst, hipStream_t s);
// launch_attention_mixed on packed rows: qkv (rows, 3 HID), out (rows, HID), clip b's keys and queries in rows row0[b] .. + frames[b]
hipError_t launch_attention_packed(const float *qkv, int HID, int heads, const int *work, int n_work, const int *frames, const int *row0,
                                   float scale, float *out, hipStream_t s);
// dst[0 .. n) (device) = host[0 .. n), carried by kernel arguments (ceil(n / 960) tiny launches): `host` is free when the call returns
struct PutWords {
    static constexpr int N = 960;
    int v[N];
};
hipError_t launch_put_words(int *dst, const int *host, long n, hipStream_t s);

// ------------------------------------------------------------------------------------------------
// audio front-end kernels (mfcc.hip; host side: mfcc.cpp)
// ------------------------------------------------------------------------------------------------
hipError_t launch_resample_polyphase(const float *x, int B, int N, const float *kern, int norig, int nnew, int width, int kw,
                                     float *out, int Nout, hipStream_t s);
hipError_t launch_stft_power(const float *x, int B, int N, int T, int hop, const float *win, const float *tw1024, const float *tw2048,
                             float *pw, int ldp, hipStream_t s);
hipError_t launch_resample_kaiser(const float *x, int B, int N, const float *win, const float *delta, int nwin, int num_table,
                                  double ratio, float *out, int Nout, int ldo, hipStream_t s);
hipError_t launch_db_topdb(float *mel, int B, long per_clip, float top_db, hipStream_t s);
// length variants (mixed passes): ns = device table of the recordings' own sample counts at the input rate
hipError_t launch_resample_polyphase_lens(const float *x, int B, int N, const int *ns, const float *kern, int norig, int nnew, int width,
                                          int kw, float *out, int Nout, hipStream_t s);
hipError_t launch_copy_samples_lens(const float *x, int B, int N, const int *ns, float *out, hipStream_t s);
hipError_t launch_resample_kaiser_lens(const float *x, int B, int N, const int *ns, const float *win, const float *delta, int nwin,
                                       int num_table, double ratio, float *out, int ldo, hipStream_t s);
hipError_t launch_mfcc_frames(const int *ns, int B, int N, int norig, int nnew, int hop, int *frames, hipStream_t s);
hipError_t launch_stft_power_lens(const float *x, int B, int N, int T, const int *ns, int norig, int nnew, int hop, const float *win,
                                  const float *tw1024, const float *tw2048, float *pw, int ldp, hipStream_t s);
hipError_t launch_db_topdb_lens(float *mel, int B, int T, int width, const int *frames, float top_db, hipStream_t s);
hipError_t launch_db_peak_lens(const float *mel, int B, int T, int width, const int *frames, float *out, hipStream_t s);
// wav sessions: rows indexed by absolute sample index
hipError_t launch_stream_rows_copy(const float *src, long lds, long off, int len, float *dst, long ldd, int B, hipStream_t s);
hipError_t launch_resample_polyphase_stream(const float *x, long ldx, long x0, long n, int B, const float *kern, int norig, int nnew, int width,
                                            int kw, float *out, long ldo, long o0, long j_lo, long j_hi, hipStream_t s);
hipError_t launch_stft_power_stream(const float *x, long ldx, long x0, long N, int B, int F, int t0, int hop, const float *win,
                                    const float *tw1024, const float *tw2048, float *pw, int ldp, hipStream_t s);
hipError_t launch_db_stream(float *mel, int B, int F, const float *peak, float *run_max, float top_db, hipStream_t s);

// ---- body_stream.hip: the staging around the window calls of a seamless body session (body_stream.cpp) ----
// [tail (B, cap, 64) rows [0, n_tail) | chunk (B, t, 64)] per clip: frames [0, Tw) -> win (B, Tw, 64), frames [next0, next0 + n_next) ->
// next (B, cap, 64) rows [0, n_next); tail != next.  Every pointer 16-byte aligned; a shape outside the buffers is hipErrorInvalidValue
hipError_t launch_stream_stage_mfcc(const float *tail, const float *chunk, float *win, float *next, int B, int n_tail, int t, int cap, int Tw,
                                    int next0, int n_next, hipStream_t s);
// codes (B, n, 2) = code rows [A, A + n) -> ring (B, RC, 2) slots r % RC; rows [v0, v0 + Hw) of ring + codes -> lat_body, lat_hand (B, Hw)
hipError_t launch_stream_emit(const int64_t *codes, int64_t *ring, int64_t *lat_body, int64_t *lat_hand, int B, int n, int A, int RC, int v0,
                              int Hw, hipStream_t s);
// dst (B, n, W) = rows [r0, r0 + n) of every clip of src (B, R, W)
hipError_t launch_stream_keep_rows(const float *src, float *dst, int B, int R, int r0, int n, int W, hipStream_t s);
// dst (S, n, W) = rows [r0, r0 + n) of stream map[s] of src (E, R, W): W a multiple of 4, both 16-byte aligned; map (S,) on the device,
// values in [0, E) (the caller's to guarantee)
hipError_t launch_stream_spread_rows(const float *src, float *dst, const int32_t *map, int S, int E, int R, int r0, int n, int W,
                                     hipStream_t s);

}  // namespace ts
