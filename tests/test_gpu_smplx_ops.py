"""Op-level tests of the batched SMPL-X forward (`csrc/smplx.hip`, `csrc/smplx.cpp`), stage by stage against float64, through the test aids of
`include/talkshow_hip_debug.h` (`ts_debug_smplx_pose_prepare / _blend / _rigid_chain / _skin / _joints_tail`, `_dims` and `_need` for the host
tables): each one production launch on the model handle's own tables, so what is tested is the device's pose offsets and mean, the three packed
GEMM operands (the folded joint regressor among them), the parents, the sparse skinning weights and the selector / landmark maps.

References.  The float64 stage functions of oracle/smplx_oracle.py (the published LBS restated: Rodrigues and pose feature, shaped and posed
vertices, rest joints, rigid chain, skinning, selector and landmarks); `test_stage_references_compose` holds their composition to the
one-piece function they were split from.  Every stage gets its inputs as fp32 arrays and its reference from those same fp32 values in float64
(the model's arrays too: `model32`), so a stage's error is its own.

Guards.  Inputs and outputs sit in the allocations of tests/test_gpu_canary.py (`Guarded`, `run_both`: NaN red zones round the inputs, a
sentinel in and round the outputs, the guarded call bit-equal to the plain one, every output element written; for the two entries that write
part of the joint list the untouched part must still hold the sentinel).

Error units and bounds (measured, not guessed: the protocol of tests/test_gpu_conv_ops.py and tests/test_gpu_frontend_ops.py).
  pose_prepare  R and the pose feature of a joint: max(1, angle), the angle's own fp32 rounding (row + mean, the norm) scales with it.  No
                documented bound of the device's sinf / cosf was at hand: NO ceiling is asserted, the bound is the measured one alone.  The
                betas and expression columns of X are copies (bit-equal), the pad columns +0.0, R of a zero axis-angle I and its feature 0.
  blend         sum |x w| + |bias| per output; ceiling (Kpad + 4) 2^-24.  The folded regressor is read back through one-hot rows of X on a
                model whose template is zero (0 + 1 w + zeros: exact) and the bias through a zero row: |got - ref| <= 2^-24 |ref| + 1e-15 of
                the float64 product, one fp32 rounding.  Derived, not measured.
  rigid_chain   rotation part of G and A: 1; G's translation and the joints: the joint's path length L_j = sum |rel|_1 from the root (the
                root's own position included); A's translation: L_j + |J_j|_1.  Ceilings in terms of the depth d of the joint (SMPL-X: at
                most 10): one level computes G_p R_j entry by entry as a 3-term fp32 sum, error <= 3 u |G_p| |R_j| <= 3 u per entry (rows and
                columns of rotations have 2-norm 1), sqrt 3 of that per row in 2-norm; a rotation carries the inherited row error on
                unchanged: d 3 sqrt 3 u.  The translation G_p.R rel + t_p is a 4-term sum of magnitude <= L_j with rel rounded once and G_p.R
                off by the above: (5 + 3 sqrt 3 d) u |rel|_1 + 4 u L_j per level, <= (5 + (4 + 3 sqrt 3) d) u L_j along the path.  A's
                translation adds one 4-term sum over G.R J_j and G.t: (4 + 3 sqrt 3 d) u more, in its unit.  (1.01 covers the higher orders.)
  skin          sum_k w_k (|A_k.R| |v| + |A_k.t|) per coordinate; ceiling (KW + 4) u: a KW-term sum for the blended transform, a 4-term
                sum for its product with [v; 1].
  joints_tail   extra joints are copies (bit-equal); landmarks: sum |b| |v|; ceiling 3 u (a 3-term sum).
  forward       ts_smplx_forward against the oracle end to end, in metres: a composition of the above, no ceiling of its own.
Each asserted bound is 2x the largest error of its stage that the first MI355X run of this file recorded (TS_MEASURED_LOG;
profiles/smplx_eval_ops_measured.jsonl: that run asserted the ceilings, or nothing where there is none), with one exception: for the
landmarks 2x the record (1.7 of the 3 roundings a 3-term sum can make) lies over the ceiling, and the ceiling is asserted.
`test_bounds_catch_defects` (CPU) applies each defect of DEFECTS to the float64 reference and shows that the bound of the stage named there misses it by at least 10x.

Bit-identity.  The stages run one after the other through the aids give the bits of ts_smplx_forward, joints and vertices.  The two loops
that production shapes never take twice — the frame chunks of the full mesh and the 65 535-frame slices of the skinning launch — run on rows
that repeat with a small odd period: every frame equals, bit for bit, the frame of its period in the first chunk / slice.
"""
import ctypes as C
import math
import time

import numpy as np
import pytest
import torch

from conftest import assert_close_measured
from oracle import smplx_oracle as SO
from test_gpu_canary import F32, F_SENT, run_both

F64 = np.float64
U = 2.0 ** -24
J = 55
PARENTS = SO.SMPLX_PARENTS
DEPTH = np.zeros(J, int)
for _j in range(1, J):
    DEPTH[_j] = DEPTH[PARENTS[_j]] + 1
D_MAX = int(DEPTH.max())
S3 = 3.0 * math.sqrt(3.0)
ROT_CEILING = 1.01 * D_MAX * S3 * U
TRANS_CEILING = 1.01 * (5 + (4 + S3) * D_MAX) * U
ATRANS_CEILING = TRANS_CEILING + 1.01 * (4 + S3 * D_MAX) * U
LMK_CEILING = 1.01 * 3 * U
# 2x the largest error of the stage in the first MI355X run's records (profiles/smplx_eval_ops_measured.jsonl; that run had no bounds yet and
# asserted the ceilings, its pose_prepare and forward lines carry an infinite bound), in the units of the docstring.  Every case passed on that run.
POSE_BOUND = 2.9e-7          # 1.409e-7: b0e10, 272 columns
BLEND_BOUND = 1.2e-6         # 5.694e-7: v700, the full mesh, N = 301 (9.6 x 2^-24 over Kpad = 896)
CHAIN_ROT_BOUND = 5.3e-7     # 2.649e-7: N = 301
CHAIN_TRANS_BOUND = 1.4e-7   # 6.537e-8: N = 301
CHAIN_ATRANS_BOUND = 1.3e-7  # 6.422e-8: N = 65
SKIN_BOUND = 2.5e-7          # 1.212e-7: v700, the full mesh
# landmarks: 1.015e-7 (the model with shared vertices) is 1.7 of the 3 roundings a 3-term sum can make, so 2x the record lies ABOVE the derived
# ceiling; the ceiling, the tighter of the two, is what is asserted
LMK_BOUND = min(2.1e-7, LMK_CEILING)
FORWARD_BOUND = 3.4e-7       # metres; 1.665e-7: the real mesh size, N = 3 (and the same frames at the chunk boundary)
TABLE_REL, TABLE_ABS = U, 1e-15


def gemm_ceiling(Kpad):
    return (Kpad + 4) * U


def skin_ceiling(KW):
    return 1.01 * (KW + 4) * U


def measured(stage, case, err, bound, ceiling=None):
    """Records err (TS_MEASURED_LOG) and asserts it under the stage's bound; the bound itself under the case's ceiling.  Until the first
    run's records exist a bound is infinite: then the ceiling is asserted, or nothing where there is none."""
    if math.isinf(bound) and ceiling is not None:
        bound = ceiling
    assert ceiling is None or bound <= ceiling, f"{stage}.{case}: bound {bound:.2e} over the ceiling {ceiling:.2e}"
    assert_close_measured(f"smplx.{stage}.{case}", np.array([err]), np.array([0.0]), bound)


def in_units(err, unit):
    """max err / unit; where the unit is 0 (nothing contributes) the error must be 0.  A NaN counts as an infinite error."""
    err, unit = np.asarray(err, F64), np.asarray(unit, F64)
    if np.isnan(err).any():
        return math.inf
    assert (err[unit == 0] == 0).all(), "a value that nothing contributes to is not exactly zero"
    return float((err[unit > 0] / unit[unit > 0]).max()) if (unit > 0).any() else 0.0


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


# ----------------------------------------------------------------------------------------------- models, inputs, float64 references
_FLOAT_KEYS = ("v_template", "shapedirs", "posedirs", "J_regressor", "lbs_weights", "pose_mean", "lmk_bary")


def model32(**kw):
    """A synthetic model whose float arrays hold fp32 values (in float64): what the device gets is what the reference computes with."""
    m = SO.synthetic_model(**kw)
    for k in _FLOAT_KEYS:
        m[k] = np.asarray(m[k], np.float32).astype(F64)
    return m


def need_of(m):
    """The vertices the joint list needs, each once, in order of first use (extra joints, then landmark corners); {0} if there are none."""
    seen = list(dict.fromkeys(np.concatenate([np.asarray(m["extra_idx"]).reshape(-1), np.asarray(m["lmk_faces"]).reshape(-1)]).tolist()))
    return np.asarray(seen if seen else [0], np.int64)


def kw_of(m):
    return max(1, int((m["lbs_weights"] != 0).sum(1).max()))


def rand_rotvecs(rng, shape, scales):
    """Axis-angle vectors of random direction; the angle of entry i is scales[i % len] (1 +- 1e-3)."""
    d = rng.standard_normal(shape + (3,))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    n = int(np.prod(shape))
    a = np.asarray(scales, F64)[np.arange(n) % len(scales)].reshape(shape) * (1.0 + 1e-3 * rng.uniform(-1, 1, shape))
    return d * a[..., None]


def rotations32(rng, N, scales=(1e-4, 0.35, math.pi)):
    """(N, J, 9) fp32 rotation matrices at the three angle scales (float64 Rodrigues, rounded once)."""
    r = rand_rotvecs(rng, (N, J), scales)
    return SO.batch_rodrigues(r.reshape(-1, 3)).reshape(N, J, 9).astype(np.float32)


def rest_joints32(rng, m, N):
    """(N, 3 J) fp32: the model's template joints, moved a little per frame as shape coefficients move them."""
    j0 = m["J_regressor"] @ m["v_template"]
    return (j0[None] + 0.01 * rng.standard_normal((N, J, 3))).reshape(N, 3 * J).astype(np.float32)


POSE_SCALES = (1e-4, 0.35, math.pi, 3 * math.pi)


def pose_rows(rng, m, N, row_ld, expr_off=165):
    """(N, row_ld) fp32 rows: the joints' angles cycle through POSE_SCALES (the hand mean comes on top); row 0 is the zero pose of every
    joint (columns of joints with a mean hold -mean, so row + mean is exactly 0); expression O(1); NaN in every column the model does not read."""
    from talkshow_amd.smplx_lbs import TALKSHOW_POSE_OFFSETS as OFF
    rows = np.full((N, row_ld), np.nan, np.float32)
    r = rand_rotvecs(rng, (N, J), POSE_SCALES).astype(np.float32)
    mean = m["pose_mean"].reshape(J, 3).astype(np.float32)
    r[0] = -mean
    for j in range(J):
        rows[:, OFF[j]:OFF[j] + 3] = r[:, j]
    rows[:, expr_off:expr_off + m["n_expr"]] = rng.standard_normal((N, m["n_expr"])).astype(np.float32)
    return rows


def pose_ref(m, betas, rows, expr_off=165, defect=None):
    """-> R (N, J, 3, 3), feature (N, 9 (J - 1)), angle (N, J), shape coefficients (N, S): float64 from the fp32 rows."""
    clean = np.nan_to_num(np.asarray(rows, F64))
    full, shape = SO.pose_and_shape_from_rows(m, betas, clean, expr_off)
    N = full.shape[0]
    if defect == "rodrigues_without_1e-8":
        with np.errstate(all="ignore"):
            R = SO.batch_rodrigues(full.reshape(-1, 3), 0.0).reshape(N, J, 3, 3)
        feat = (R[:, 1:] - np.eye(3)).reshape(N, -1)
    else:
        R, feat = SO.rodrigues_pose_feature(full)
    if defect == "R_transposed_on_one_joint":
        R = R.copy()
        R[:, 37] = R[:, 37].transpose(0, 2, 1)
    return R, feat, np.linalg.norm(full.reshape(N, J, 3), axis=-1), shape


def pose_error(R_got, R_ref, angle):
    unit = np.maximum(1.0, angle)[:, :, None, None]
    return in_units(np.abs(np.asarray(R_got, F64).reshape(R_ref.shape) - R_ref), np.broadcast_to(unit, R_ref.shape))


_TABLES = {}


def blend_tables(m, which, defect=None):
    """Cached per model: (W (rows, S + P), bias (rows,)) of GEMM `which` as float64: 0 = the folded joint regressor as the device must hold it, fp32 of the
    float64 product; 1 / 2 = [shapedirs | posedirs^T] and the template of the needed / of all vertices."""
    key = (id(m), which, defect)
    if key not in _TABLES:
        _TABLES[key] = (m, _blend_tables(m, which, defect))              # m is kept so that its id stays its own
    return _TABLES[key][1]


def _blend_tables(m, which, defect):
    V, S = m["v_template"].shape[0], m["n_betas"] + m["n_expr"]
    P = (J - 1) * 9
    if which == 0:
        sd = m["shapedirs"]
        if defect == "regressor_drops_a_shape_component":
            sd = sd.copy()
            sd[:, :, 3] = 0.0
        W = np.zeros((3 * J, S + P))
        W[:, :S] = np.einsum("jv,vcs->jcs", m["J_regressor"], sd).reshape(3 * J, S).astype(np.float32)
        return W, (m["J_regressor"] @ m["v_template"]).reshape(-1).astype(np.float32).astype(F64)
    vs = need_of(m) if which == 1 else np.arange(V)
    W = np.concatenate([m["shapedirs"][vs].reshape(-1, S), m["posedirs"].reshape(P, V, 3)[:, vs].reshape(P, -1).T], axis=1)
    return W, m["v_template"][vs].reshape(-1)


def blend_ref(m, which, X, defect=None):
    """-> (values, units sum |x w| + |bias|) for X (N, Kpad) fp32."""
    W, b = blend_tables(m, which, defect)
    x = np.asarray(X, F64)[:, :W.shape[1]]
    return x @ W.T + b, np.abs(x) @ np.abs(W).T + np.abs(b)


def blend_inputs(rng, m, N, Kpad):
    """(N, Kpad) fp32 as pose_prepare lays it out: betas ~ 0.8, expression ~ 1, R - I of rotations at the three scales, zeros in the pad."""
    S = m["n_betas"] + m["n_expr"]
    X = np.zeros((N, Kpad), np.float32)
    X[:, :m["n_betas"]] = 0.8 * rng.standard_normal((N, m["n_betas"]))
    X[:, m["n_betas"]:S] = rng.standard_normal((N, m["n_expr"]))
    X[:, S:S + 9 * (J - 1)] = (rotations32(rng, N)[:, 1:].astype(F64) - np.eye(3).reshape(9)).reshape(N, -1)
    return X


def chain_ref(rot, jrest, defect=None):
    """rot (N, J, 9), jrest (N, 3 J) fp32 -> G, A (N, J, 3, 4), joints (N, J, 3) and the units: path length L (N, J), |J_j|_1 (N, J)."""
    N = rot.shape[0]
    R, Jr = np.asarray(rot, F64).reshape(N, J, 3, 3), np.asarray(jrest, F64).reshape(N, J, 3)
    parents = PARENTS.copy()
    if defect == "parent_off_by_one":
        parents[40] -= 1
    G, A, joints = SO.rigid_chain(R, Jr, parents)
    if defect == "A_without_R_J":
        A = G.copy()
    rel = Jr.copy()
    rel[:, 1:] -= Jr[:, PARENTS[1:]]
    L = np.abs(rel).sum(-1)
    for j in range(1, J):
        L[:, j] += L[:, PARENTS[j]]
    return G[:, :, :3], A[:, :, :3], joints, L, np.abs(Jr).sum(-1)


def chain_errors(G, A, joints, ref):
    """-> (rotation, translation, A's translation) errors in their units."""
    Gr, Ar, jr, L, Ja = ref
    N = Gr.shape[0]
    G, A, joints = (np.asarray(a, F64).reshape(s) for a, s in ((G, (N, J, 3, 4)), (A, (N, J, 3, 4)), (joints, (N, J, 3))))
    rot = max(float(np.abs(G[..., :3] - Gr[..., :3]).max()), float(np.abs(A[..., :3] - Ar[..., :3]).max()))
    Lu = np.broadcast_to(L[:, :, None], (N, J, 3))
    tr = max(in_units(np.abs(G[..., 3] - Gr[..., 3]), Lu), in_units(np.abs(joints - jr), Lu))
    at = in_units(np.abs(A[..., 3] - Ar[..., 3]), Lu + Ja[:, :, None])
    return rot, tr, at


def transforms32(rng, m, N):
    """(N, J, 12) fp32 relative transforms A of random poses: the float64 chain, rounded once."""
    return chain_ref(rotations32(rng, N, (0.35, 1.0, math.pi)), rest_joints32(rng, m, N))[1].reshape(N, J, 12).astype(np.float32)


def skin_ref(m, vs, vposed, A, defect=None):
    """vposed (N, n, 3), A (N, J, 12) fp32, the weights of vertices vs -> (values (N, n, 3), units)."""
    w = m["lbs_weights"][vs]
    if defect == "last_bone_dropped":
        w = w.copy()
        for i in range(w.shape[0]):
            nz = np.flatnonzero(w[i])
            if nz.size > 1:
                w[i, nz[-1]] = 0.0
    N = A.shape[0]
    A = np.asarray(A, F64).reshape(N, J, 3, 4)
    v = np.asarray(vposed, F64).reshape(N, -1, 3)
    vh = np.concatenate([v, np.ones(v.shape[:2] + (1,))], -1)
    out = np.einsum("vj,bjrc,bvc->bvr", w, A, vh)
    unit = np.einsum("vj,bjrc,bvc->bvr", w, np.abs(A), np.abs(vh))
    return out, unit


def tail_ref(m, vs, defect=None):
    """vs (N, U, 3) fp32 in slot order -> extra (N, n_extra, 3), landmarks (N, n_lmk, 3), landmark units."""
    need = need_of(m)
    slot = {int(v): i for i, v in enumerate(need)}
    v = np.asarray(vs, F64)
    ex = v[:, [slot[int(i)] for i in np.asarray(m["extra_idx"]).reshape(-1)]] if len(m["extra_idx"]) else np.zeros((v.shape[0], 0, 3))
    faces = np.asarray(m["lmk_faces"]).reshape(-1, 3)
    if faces.shape[0] == 0:
        return ex, np.zeros((v.shape[0], 0, 3)), np.zeros((v.shape[0], 0, 3))
    tri = v[:, np.vectorize(slot.get)(faces)]
    b = m["lmk_bary"][:, [1, 2, 0]] if defect == "barycentric_permuted" else m["lmk_bary"]
    return ex, np.einsum("blfi,lf->bli", tri, b), np.einsum("blfi,lf->bli", np.abs(tri), np.abs(m["lmk_bary"]))


# ----------------------------------------------------------------------------------------------- GPU plumbing
class Handle:
    def __init__(self, _lib, m, with_vertices):
        from talkshow_amd.smplx_lbs import SMPLXLayer
        self.m, self.layer = m, SMPLXLayer(m, with_vertices=with_vertices)
        self.h = self.layer._h
        d = (C.c_int32 * 5)()
        _lib.check(_lib.load().ts_debug_smplx_dims(self.h, d))
        self.Kpad, self.U, self.KW, self.NJ, self.chunk = (int(x) for x in d)
        need = (C.c_int32 * self.U)()
        _lib.check(_lib.load().ts_debug_smplx_need(self.h, need))
        self.need = np.asarray(list(need), np.int64)
        self.V = m["v_template"].shape[0]


MODELS = {
    "v700": dict(seed=3, V=700),                                        # the shapes of the real model's coefficients, full mesh
    "real": dict(seed=4, V=10475, n_betas=10, n_expr=10),               # the real mesh size, full mesh: 31 425 GEMM columns
    "b10e10": dict(seed=5, V=200, n_betas=10, n_expr=10),
    "b26e0": dict(seed=6, V=200, n_betas=26, n_expr=0),                 # S + P = 512: no pad columns
    "b0e10": dict(seed=7, V=200, n_betas=0, n_expr=10),
    "kw1": dict(seed=8, V=333, n_betas=10, n_expr=10, max_bones=1),
    "no_extra": dict(seed=10, V=200, n_betas=10, n_expr=10, n_extra=0),
    "no_lmk": dict(seed=11, V=200, n_betas=10, n_expr=10, n_lmk=0),
    "bare": dict(seed=12, V=200, n_betas=10, n_expr=10, n_extra=0, n_lmk=0),
    "shared": dict(seed=13, V=200, n_betas=10, n_expr=10, shared=6),
}
FULL_MESH = ("v700", "real", "kw1", "allbones")


def model_by_name(name):
    if name == "allbones":                                              # a vertex of the needed subset weighted on all 55 bones
        kw = dict(seed=9, V=333, n_betas=10, n_expr=10)
        return model32(all_bones_vertex=int(SO.synthetic_model(**kw)["extra_idx"][0]), **kw)
    return model32(**MODELS[name])


@pytest.fixture(scope="module")
def hip():
    from talkshow_amd import _lib
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    lib = _lib.load()
    cache = {}

    def handle(name):
        if name not in cache:
            cache[name] = Handle(_lib, model_by_name(name), name in FULL_MESH)
        return cache[name]

    yield _lib, lib, handle
    torch.cuda.synchronize()
    cache.clear()


def run_pose(hip, H, betas, bpr, rows, expr_off=165):
    _lib, lib, _ = hip
    N, ld = rows.shape
    r = run_both(lambda p: _lib.check(lib.ts_debug_smplx_pose_prepare(H.h, p["betas"], bpr, p["rows"], ld, expr_off, N, p["rot"], p["X"],
                                                                      _lib.stream_ptr())),
                 {"betas": (betas, F32), "rows": (rows, F32)}, {"rot": ((N, J, 9), F32), "X": ((N, H.Kpad), F32)})
    return r["rot"].cpu().numpy(), r["X"].cpu().numpy()


def run_blend(hip, H, which, X):
    _lib, lib, _ = hip
    N, n = X.shape[0], 3 * (J, H.U, H.V)[which]
    r = run_both(lambda p: _lib.check(lib.ts_debug_smplx_blend(H.h, which, p["X"], N, p["out"], _lib.stream_ptr())),
                 {"X": (X, F32)}, {"out": ((N, n), F32)})
    return r["out"].cpu().numpy()


def run_chain(hip, H, rot, jrest):
    """-> G, A (N, J, 12), joints (N, NJ, 3): entries J .. NJ - 1 must still hold the sentinel."""
    _lib, lib, _ = hip
    N = rot.shape[0]
    r = run_both(lambda p: _lib.check(lib.ts_debug_smplx_rigid_chain(H.h, p["rot"], p["jrest"], N, p["G"], p["A"], p["joints"], _lib.stream_ptr())),
                 {"rot": (rot, F32), "jrest": (jrest, F32)}, {"G": ((N, J, 12), F32), "A": ((N, J, 12), F32), "joints": ((N, H.NJ, 3), F32)},
                 written=("G", "A"))
    jo = r["joints"].cpu().numpy()
    assert (bits(jo[:, :J]) != F_SENT).all(), "a chain joint was never written"
    assert (bits(jo[:, J:]) == F_SENT).all(), "the chain wrote into the selector's part of the joint list"
    return r["G"].cpu().numpy(), r["A"].cpu().numpy(), jo


def run_skin(hip, H, full, vposed, A):
    _lib, lib, _ = hip
    N = A.shape[0]
    r = run_both(lambda p: _lib.check(lib.ts_debug_smplx_skin(H.h, full, p["v"], p["A"], N, p["out"], _lib.stream_ptr())),
                 {"v": (vposed, F32), "A": (A, F32)}, {"out": (vposed.shape, F32)})
    return r["out"].cpu().numpy()


def run_tail(hip, H, vs):
    """-> joints (N, NJ, 3): entries 0 .. J - 1 must still hold the sentinel."""
    _lib, lib, _ = hip
    N = vs.shape[0]
    r = run_both(lambda p: _lib.check(lib.ts_debug_smplx_joints_tail(H.h, p["vs"], N, p["joints"], _lib.stream_ptr())),
                 {"vs": (vs, F32)}, {"joints": ((N, H.NJ, 3), F32)}, written=())
    jo = r["joints"].cpu().numpy()
    assert (bits(jo[:, :J]) == F_SENT).all(), "the selector wrote into the chain's part of the joint list"
    assert (bits(jo[:, J:]) != F_SENT).all(), "an extra joint or landmark was never written"
    return jo


def run_forward(hip, H, betas, bpr, rows, want_verts, expr_off=165, guarded=True):
    """ts_smplx_forward -> joints (N, NJ, 3), verts (N, V, 3) or None as device tensors."""
    _lib, lib, _ = hip
    N, ld = rows.shape
    outs = {"joints": ((N, H.NJ, 3), F32)}
    if want_verts:
        outs["verts"] = ((N, H.V, 3), F32)
    r = run_both(lambda p: _lib.check(lib.ts_smplx_forward(H.h, p["betas"], bpr, p["rows"], ld, expr_off, N, p["joints"], p.get("verts"),
                                                           _lib.stream_ptr())),
                 {"betas": (betas, F32), "rows": (rows, F32)}, outs)
    return r["joints"], r.get("verts")


# ----------------------------------------------------------------------------------------------- pose_prepare
@pytest.mark.gpu
@pytest.mark.parametrize("row_ld,bpr", [(265, 0), (272, 1)])
@pytest.mark.parametrize("name", ["v700", "b10e10", "b26e0", "b0e10"])
def test_pose_prepare(hip, name, row_ld, bpr):
    """Angles of 1e-4, 0.35, pi and 3 pi on every joint in turn, the hand mean on top; row 0 the zero pose; NaN in the columns nobody reads
    (with 272 columns: the pad; with no expression: everything from 165 on); one betas row for all or one per pose row."""
    H = hip[2](name)
    m, N = H.m, 9
    S = m["n_betas"] + m["n_expr"]
    assert H.Kpad == -(-(S + 486) // 32) * 32 and (H.Kpad == S + 486) == (name == "b26e0")
    rng = np.random.default_rng(row_ld + S)
    rows = pose_rows(rng, m, N, row_ld)
    betas = (0.8 * rng.standard_normal((N if bpr else 1, max(m["n_betas"], 1)))).astype(np.float32)[:, :m["n_betas"]]
    betas_dev = betas if betas.size else np.zeros((1, 1), np.float32)           # a model without betas still gets a valid pointer
    rot, X = run_pose(hip, H, betas_dev, bpr, rows)
    R, feat, angle, shape = pose_ref(m, betas.astype(F64), rows)
    assert angle[0].max() == 0 and angle.max() > 9.0
    assert np.array_equal(bits(X[:, :m["n_betas"]]), bits(np.broadcast_to(betas, (N, m["n_betas"])))), "X's betas columns are no copies"
    assert np.array_equal(bits(X[:, m["n_betas"]:S]), bits(rows[:, 165:165 + m["n_expr"]])), "X's expression columns are no copies"
    assert (bits(X[:, S + 486:]) == 0).all(), "a pad column is not +0.0"
    assert np.array_equal(rot[0].reshape(J, 3, 3), np.broadcast_to(np.eye(3, dtype=np.float32), (J, 3, 3))), "R of the zero axis-angle is not I"
    assert (X[0, S:S + 486] == 0).all(), "the pose feature of the zero pose is not 0"
    e = max(pose_error(rot, R, angle), pose_error(X[:, S:S + 486].reshape(N, J - 1, 3, 3), feat.reshape(N, J - 1, 3, 3), angle[:, 1:]))
    measured("pose_prepare", f"{name}.ld{row_ld}", e, POSE_BOUND)


@pytest.mark.gpu
def test_rows_narrower_than_the_model_reads_are_refused(hip):
    """165-column rows (poses, no expression) and expression at column 200 of 265: refused by the Python layer before any call and by both
    entries before any launch (the outputs keep their fill)."""
    from talkshow_amd.smplx_lbs import SMPLXLayer, TALKSHOW_POSE_OFFSETS
    _lib, lib, handle = hip
    H = handle("v700")
    betas = torch.zeros(300, device="cuda")
    with pytest.raises(ValueError, match="165 columns"):
        H.layer.joints(betas, torch.zeros(4, 165, device="cuda"))
    with pytest.raises(ValueError, match="265 columns"):
        SMPLXLayer(H.m, expr_offset=200).joints(betas, torch.zeros(4, 265, device="cuda"))
    rows = torch.zeros(4, 265, device="cuda")
    joints = torch.full((4, H.NJ, 3), 7.0, device="cuda")
    rot, X = torch.full((4, J, 9), 7.0, device="cuda"), torch.full((4, H.Kpad), 7.0, device="cuda")
    s = _lib.stream_ptr()
    for ld, off, word in ((165, 165, b"165 columns"), (265, 200, b"265 columns"), (164, 0, b"164 columns"), (265, -1, b"negative expression offset")):
        assert lib.ts_smplx_forward(H.h, _lib.dptr(betas), 0, _lib.dptr(rows), ld, off, 4, _lib.dptr(joints), None, s) != 0
        assert b"ts_smplx_forward" in lib.ts_last_error() and word in lib.ts_last_error()
        assert lib.ts_debug_smplx_pose_prepare(H.h, _lib.dptr(betas), 0, _lib.dptr(rows), ld, off, 4, _lib.dptr(rot), _lib.dptr(X), s) != 0
        assert b"ts_debug_smplx_pose_prepare" in lib.ts_last_error() and word in lib.ts_last_error()
    torch.cuda.synchronize()
    assert bool((joints == 7.0).all()) and bool((rot == 7.0).all()) and bool((X == 7.0).all())
    # a model without expression reads 165 columns and no more
    H0 = handle("b26e0")
    j = H0.layer.joints(np.zeros(26, np.float32), np.zeros((2, 165), np.float32))
    assert j.shape == (2, H0.NJ, 3) and bool(torch.isfinite(j).all())
    bad = TALKSHOW_POSE_OFFSETS.copy()
    bad[7] = -3
    with pytest.raises(RuntimeError, match="negative pose_src_offset"):
        SMPLXLayer(H0.m, pose_offsets=bad)


# ----------------------------------------------------------------------------------------------- the three GEMMs
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 33, 301])
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("name", ["v700", "real"])
def test_blend(hip, name, which, N):
    """Rest joints (165 columns), needed vertices (3 U) and the full mesh (2100 and 31 425 columns, the latter odd) over one row, a ragged
    count and more than two row tiles."""
    H = hip[2](name)
    X = blend_inputs(np.random.default_rng(100 * which + N), H.m, N, H.Kpad)
    got = run_blend(hip, H, which, X)
    ref, unit = blend_ref(H.m, which, X)
    assert got.shape == ref.shape and (which != 2 or name != "real" or ref.shape[1] == 31425)
    measured("blend", f"{name}.which{which}.n{N}", in_units(np.abs(got - ref), unit), BLEND_BOUND, gemm_ceiling(H.Kpad))


@pytest.mark.gpu
def test_folded_regressor_read_back(hip):
    """One-hot rows of X on a model whose template is zero return the columns of the device's folded regressor exactly; a zero row on the
    model with its template returns the folded template.  Both equal fp32 of the float64 products."""
    from talkshow_amd.smplx_lbs import SMPLXLayer
    _lib, lib, handle = hip
    m = dict(model_by_name("b10e10"))
    m["v_template"] = np.zeros_like(m["v_template"])
    H = Handle(_lib, m, False)
    S = 20
    X = np.zeros((S + 1, H.Kpad), np.float32)
    X[np.arange(S), np.arange(S)] = 1.0
    got = run_blend(hip, H, 0, X)
    assert (got[S] == 0).all()
    ref = np.einsum("jv,vcs->jcs", m["J_regressor"], m["shapedirs"]).reshape(3 * J, S).T
    bad = np.abs(got[:S].astype(F64) - ref) > TABLE_REL * np.abs(ref) + TABLE_ABS
    assert not bad.any(), f"folded regressor: {int(bad.sum())} entries off, the worst by {np.abs(got[:S] - ref).max():.3e} at {np.argwhere(bad)[:4].tolist()}"
    Hn = handle("b10e10")
    b = run_blend(hip, Hn, 0, np.zeros((1, Hn.Kpad), np.float32))[0]
    ref = (Hn.m["J_regressor"] @ Hn.m["v_template"]).reshape(-1)
    assert (np.abs(b.astype(F64) - ref) <= TABLE_REL * np.abs(ref) + TABLE_ABS).all(), "the folded template is not fp32 of the float64 product"


# ----------------------------------------------------------------------------------------------- rigid chain
@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 63, 64, 65, 301])
def test_rigid_chain(hip, N):
    """One thread per frame in blocks of 64: one frame, one short of a block, a block, one over, several blocks."""
    H = hip[2]("b10e10")
    rng = np.random.default_rng(N)
    rot, jrest = rotations32(rng, N), rest_joints32(rng, H.m, N)
    G, A, jo = run_chain(hip, H, rot, jrest)
    assert np.array_equal(bits(jo[:, :J]), bits(G.reshape(N, J, 3, 4)[..., 3])), "the joints are not G's translation"
    assert np.array_equal(bits(G.reshape(N, J, 3, 4)[..., :3]), bits(A.reshape(N, J, 3, 4)[..., :3])), "A's rotation is not G's"
    e_rot, e_tr, e_at = chain_errors(G, A, jo[:, :J], chain_ref(rot, jrest))
    measured("chain_rot", f"n{N}", e_rot, CHAIN_ROT_BOUND, ROT_CEILING)
    measured("chain_trans", f"n{N}", e_tr, CHAIN_TRANS_BOUND, TRANS_CEILING)
    measured("chain_atrans", f"n{N}", e_at, CHAIN_ATRANS_BOUND, ATRANS_CEILING)


# ----------------------------------------------------------------------------------------------- skinning
@pytest.mark.gpu
@pytest.mark.parametrize("full", [0, 1])
@pytest.mark.parametrize("name", ["kw1", "v700", "allbones"])
def test_skin(hip, name, full):
    """One bone per vertex (KW = 1), up to 4, and a needed vertex weighted on all 55 bones (KW = 55); vertex counts that are no multiple of
    the block of 128 (and, with 333 and 700 vertices, more than one block)."""
    H = hip[2](name)
    m = H.m
    assert H.KW == kw_of(m) == {"kw1": 1, "v700": 4, "allbones": 55}[name]
    vs = np.arange(H.V) if full else H.need
    assert len(vs) % 128 != 0 and (not full or len(vs) > 128)
    if name == "allbones":
        assert (m["lbs_weights"][H.need[0]] != 0).all()
    N = 5
    rng = np.random.default_rng(len(vs))
    A = transforms32(rng, m, N)
    vposed = (m["v_template"][vs][None] + 0.01 * rng.standard_normal((N, len(vs), 3))).astype(np.float32)
    got = run_skin(hip, H, full, vposed, A)
    ref, unit = skin_ref(m, vs, vposed, A)
    measured("skin", f"{name}.full{full}", in_units(np.abs(got - ref), unit), SKIN_BOUND, skin_ceiling(H.KW))


# ----------------------------------------------------------------------------------------------- selector and landmarks
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["no_extra", "no_lmk", "shared", "b10e10"])
def test_joints_tail(hip, name):
    H = hip[2](name)
    m = H.m
    n_extra, n_lmk = len(m["extra_idx"]), len(m["lmk_faces"])
    assert H.NJ == J + n_extra + n_lmk
    assert np.array_equal(H.need, need_of(m)) and len(set(H.need.tolist())) == H.U, "the needed vertices are not de-duplicated in order of first use"
    if name == "shared":
        f, e = np.asarray(m["lmk_faces"]), np.asarray(m["extra_idx"])
        assert (f[:6, 0] == e[:6]).all() and (f[1:6, 1] == f[0:5, 2]).all(), "the shared vertices were not forced"
        assert H.U <= n_extra + 3 * n_lmk - 11
    N = 3
    vs = (0.5 * np.random.default_rng(H.U).standard_normal((N, H.U, 3))).astype(np.float32)
    jo = run_tail(hip, H, vs)
    ex, lm, unit = tail_ref(m, vs)
    assert np.array_equal(bits(jo[:, J:J + n_extra]), bits(ex)), "an extra joint is no copy of its vertex"
    measured("landmarks", name, in_units(np.abs(jo[:, J + n_extra:] - lm), unit), LMK_BOUND, LMK_CEILING)


# ----------------------------------------------------------------------------------------------- composition and edges through ts_smplx_forward
def forward_inputs(name, m, N, sigma=0.35):
    rng = np.random.default_rng([N, len(name)])
    rows = (rng.standard_normal((N, 265)) * sigma).astype(np.float32)
    rows[0, 3:9] = 0.0
    rows[:, 165:] *= np.float32(3.0)
    return (0.8 * rng.standard_normal(m["n_betas"])).astype(np.float32), rows


@pytest.mark.gpu
def test_stages_chained_equal_production(hip):
    """pose_prepare, the three GEMMs, the chain, both skinning launches and the selector one after the other through the aids = the bits of
    ts_smplx_forward, joints and vertices."""
    H = hip[2]("v700")
    N = 7
    betas, rows = forward_inputs("v700", H.m, N)
    pj, pv = run_forward(hip, H, betas, 0, rows, True)
    rot, X = run_pose(hip, H, betas, 0, rows)
    jrest = run_blend(hip, H, 0, X)
    G, A, jo = run_chain(hip, H, rot, jrest)
    vs = run_skin(hip, H, 0, run_blend(hip, H, 1, X).reshape(N, H.U, 3), A)
    tail = run_tail(hip, H, vs)
    verts = run_skin(hip, H, 1, run_blend(hip, H, 2, X).reshape(N, H.V, 3), A)
    joints = np.concatenate([jo[:, :J], tail[:, J:]], axis=1)
    assert np.isfinite(pj.cpu().numpy()).all() and np.isfinite(pv.cpu().numpy()).all()
    assert np.array_equal(bits(joints), bits(pj.cpu().numpy())), "the stages chained differ from the production entry (joints)"
    assert np.array_equal(bits(verts), bits(pv.cpu().numpy())), "the stages chained differ from the production entry (vertices)"


@pytest.mark.gpu
def test_full_mesh_at_the_real_size(hip):
    """V = 10475 with vertices, N = 3, against the oracle, in metres."""
    H = hip[2]("real")
    betas, rows = forward_inputs("real", H.m, 3)
    j, v = run_forward(hip, H, betas, 0, rows, True)
    rj, rv = SO.smplx_forward(H.m, betas.astype(F64), rows.astype(F64))
    assert v.shape == (3, 10475, 3) and j.shape == (3, 127, 3)
    e = max(float(np.abs(j.cpu().numpy() - rj).max()), float(np.abs(v.cpu().numpy() - rv).max()))
    measured("forward", "real.n3", e, FORWARD_BOUND)


@pytest.mark.gpu
def test_model_without_extra_joints_and_landmarks(hip):
    """n_extra = n_lmk = 0: the joints are the 55 chain joints, nothing else is launched."""
    H = hip[2]("bare")
    assert H.NJ == J and H.U == 1
    betas, rows = forward_inputs("bare", H.m, 4)
    j, _ = run_forward(hip, H, betas, 0, rows, False)
    rj, _ = SO.smplx_forward(H.m, betas.astype(F64), rows.astype(F64))
    assert rj.shape == (4, J, 3)
    measured("forward", "bare.n4", float(np.abs(j.cpu().numpy() - rj).max()), FORWARD_BOUND)


def periodic_rows(name, m, N, p):
    betas, rows = forward_inputs(name, m, p)
    return betas, rows, np.ascontiguousarray(rows[np.arange(N) % p])


def same_as_first_period(t, p):
    """Every frame of t (N, ...) equals, bit for bit, frame n % p (compared on the device)."""
    b = t.reshape(t.shape[0], -1).view(torch.int32)
    n = (b.shape[0] // p) * p
    whole = bool((b[:n].view(-1, p, b.shape[1]) == b[:p][None]).all())
    return whole and bool((b[n:] == b[:b.shape[0] - n]).all())


@pytest.mark.gpu
def test_full_mesh_chunk_boundary(hip):
    """Two frames more than one chunk of the full-mesh loop (2 135 frames at 10 475 vertices), rows of period 3: the second trip offsets X, A
    and the output; every frame on both sides of the boundary must be its period's frame, and the period's frames the oracle's."""
    H = hip[2]("real")
    assert H.chunk == (256 << 20) // (10475 * 12) == 2135
    N, p = H.chunk + 2, 3
    assert H.chunk < N and N % p != 0
    betas, rows_p, rows = periodic_rows("real", H.m, N, p)
    t0 = time.perf_counter()
    j, v = run_forward(hip, H, betas, 0, rows, True)
    assert same_as_first_period(v, p), "a frame of the full mesh differs from the frame of its period"
    assert same_as_first_period(j, p), "a frame's joints differ from the joints of its period"
    rj, rv = SO.smplx_forward(H.m, betas.astype(F64), rows_p.astype(F64))
    e = max(float(np.abs(j[:p].cpu().numpy() - rj).max()), float(np.abs(v[:p].cpu().numpy() - rv).max()),
            float(np.abs(v[N - p:].cpu().numpy() - rv[np.arange(N - p, N) % p]).max()))
    print(f"\n[time] chunk boundary, N = {N}: {time.perf_counter() - t0:.2f} s")
    measured("forward", "real.chunk_boundary", e, FORWARD_BOUND)


@pytest.mark.gpu
def test_skin_slices_past_65535_frames(hip):
    """Joints only, N = 65 537: frames ride on grid.y of the skinning launch, the second slice holds two frames.  Rows of period 5."""
    H = hip[2]("b10e10")
    N, p = 65537, 5
    betas, rows_p, rows = periodic_rows("b10e10", H.m, N, p)
    t0 = time.perf_counter()
    j, _ = run_forward(hip, H, betas, 0, rows, False)
    assert same_as_first_period(j, p), "a frame's joints differ from the joints of its period"
    rj, _ = SO.smplx_forward(H.m, betas.astype(F64), rows_p.astype(F64))
    e = max(float(np.abs(j[:p].cpu().numpy() - rj).max()), float(np.abs(j[N - p:].cpu().numpy() - rj[np.arange(N - p, N) % p]).max()))
    print(f"\n[time] skin slices, N = {N}: {time.perf_counter() - t0:.2f} s")
    measured("forward", "b10e10.n65537", e, FORWARD_BOUND)


# ----------------------------------------------------------------------------------------------- CPU: the references, the bounds
def _smplx_forward_in_one_piece(model, betas, rows):
    """oracle/smplx_oracle.py::smplx_forward as it stood before it was split into stage functions."""
    rows = np.asarray(rows, np.float64)
    N = rows.shape[0]
    full_pose, expr = SO.full_pose_from_rows(rows)
    full_pose = full_pose + model["pose_mean"][None]
    betas = np.broadcast_to(np.asarray(betas, np.float64).reshape(-1, model["n_betas"]), (N, model["n_betas"]))
    shape = np.concatenate([betas, expr[:, :model["n_expr"]]], axis=1)
    v_shaped = model["v_template"][None] + np.einsum("bl,mkl->bmk", shape, model["shapedirs"])
    Jr = np.einsum("bik,ji->bjk", v_shaped, model["J_regressor"])
    nj = Jr.shape[1]
    R = SO.batch_rodrigues(full_pose.reshape(-1, 3)).reshape(N, nj, 3, 3)
    pose_feature = (R[:, 1:] - np.eye(3)).reshape(N, -1)
    v_posed = v_shaped + (pose_feature @ model["posedirs"]).reshape(N, -1, 3)
    parents = model["parents"]
    rel = Jr.copy()
    rel[:, 1:] -= Jr[:, parents[1:]]
    T = np.zeros((N, nj, 4, 4))
    T[:, :, :3, :3] = R
    T[:, :, :3, 3] = rel
    T[:, :, 3, 3] = 1
    G = [T[:, 0]]
    for j in range(1, nj):
        G.append(G[parents[j]] @ T[:, j])
    G = np.stack(G, 1)
    posed_joints = G[:, :, :3, 3]
    Jh = np.concatenate([Jr, np.zeros((N, nj, 1))], -1)[..., None]
    A = G.copy()
    A[:, :, :, 3:] -= G @ Jh
    Tv = np.einsum("vj,bjrc->bvrc", model["lbs_weights"], A)
    vh = np.concatenate([v_posed, np.ones((N, v_posed.shape[1], 1))], -1)
    verts = np.einsum("bvrc,bvc->bvr", Tv, vh)[..., :3]
    extra = verts[:, model["extra_idx"]]
    tri = verts[:, model["lmk_faces"]]
    lmk = np.einsum("blfi,lf->bli", tri, model["lmk_bary"])
    return np.concatenate([posed_joints, extra, lmk], axis=1), verts


def test_stage_references_compose():
    """The stage functions composed = the one-piece function to 1e-12, for the default model and a variant; the default model's arrays are what
    they were (two keyword arguments at their defaults change nothing); the test's own stage references agree with the oracle's."""
    for kw in (dict(seed=1, V=256), dict(seed=2, V=200, n_betas=10, n_expr=10, shared=4)):
        m = SO.synthetic_model(**kw)
        rng = np.random.default_rng(0)
        rows = rng.standard_normal((4, 265)) * 0.5
        betas = rng.standard_normal(m["n_betas"])
        j1, v1 = SO.smplx_forward(m, betas, rows)
        j0, v0 = _smplx_forward_in_one_piece(m, betas, rows)
        assert np.abs(j1 - j0).max() <= 1e-12 and np.abs(v1 - v0).max() <= 1e-12
    a, b = SO.synthetic_model(seed=1, V=256), SO.synthetic_model(seed=1, V=256, all_bones_vertex=None, shared=0)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    # the references of this file on one model: stage by stage = the oracle end to end
    m = model32(seed=2, V=200, n_betas=10, n_expr=10, shared=4)
    betas, rows = forward_inputs("x", m, 3)
    R, feat, _, shape = pose_ref(m, betas.astype(F64), rows)
    X = np.concatenate([shape, feat], axis=1)
    need = need_of(m)
    jrest = blend_ref(m, 0, X)[0]
    Gr, Ar, joints, L, _ = chain_ref(R.reshape(3, J, 9), jrest)
    assert (L >= np.linalg.norm(joints - joints[:, :1], axis=-1) - 1e-12).all()
    vs, _ = skin_ref(m, need, blend_ref(m, 1, X)[0].reshape(3, -1, 3), Ar.reshape(3, J, 12))
    ex, lm, _ = tail_ref(m, vs)
    rj, rv = SO.smplx_forward(m, betas.astype(F64), rows.astype(F64))
    # the folded regressor is rounded to fp32 in blend_tables: its rounding moves the joints by ~1e-9 m
    assert np.abs(np.concatenate([joints, ex, lm], axis=1) - rj).max() <= 1e-7
    full, _ = skin_ref(m, np.arange(200), blend_ref(m, 2, X)[0].reshape(3, -1, 3), Ar.reshape(3, J, 12))
    assert np.abs(full - rv).max() <= 1e-7


# defect -> the stage whose bound catches it
DEFECTS = {"rodrigues_without_1e-8": "pose_prepare", "R_transposed_on_one_joint": "pose_prepare", "parent_off_by_one": "chain_trans",
           "A_without_R_J": "chain_atrans", "last_bone_dropped": "skin", "barycentric_permuted": "landmarks",
           "regressor_drops_a_shape_component": "blend"}


def test_bounds_catch_defects():
    """Each defect, applied to the float64 reference on inputs of the GPU tests, moves the result by at least 10x the bound of its stage."""
    m = model_by_name("b10e10")
    rng = np.random.default_rng(1)
    moved = {}
    rows = pose_rows(rng, m, 9, 272)
    betas = np.zeros((1, 10))
    R, _, angle, _ = pose_ref(m, betas, rows)
    for d in ("rodrigues_without_1e-8", "R_transposed_on_one_joint"):
        moved[d] = pose_error(pose_ref(m, betas, rows, defect=d)[0], R, angle)
    rot, jrest = rotations32(rng, 5), rest_joints32(rng, m, 5)
    ref = chain_ref(rot, jrest)
    for d, k in (("parent_off_by_one", 1), ("A_without_R_J", 2)):
        bad = chain_ref(rot, jrest, d)
        moved[d] = chain_errors(np.asarray(bad[0]), np.asarray(bad[1]), bad[2], ref)[k]
    need = need_of(m)
    A = transforms32(rng, m, 2)
    vp = (m["v_template"][need][None] + 0.01 * rng.standard_normal((2, need.size, 3))).astype(np.float32)
    sref, unit = skin_ref(m, need, vp, A)
    moved["last_bone_dropped"] = in_units(np.abs(skin_ref(m, need, vp, A, "last_bone_dropped")[0] - sref), unit)
    vs = (0.5 * rng.standard_normal((3, need.size, 3))).astype(np.float32)
    _, lm, unit = tail_ref(m, vs)
    moved["barycentric_permuted"] = in_units(np.abs(tail_ref(m, vs, "barycentric_permuted")[1] - lm), unit)
    X = blend_inputs(rng, m, 33, 512)
    bref, unit = blend_ref(m, 0, X)
    moved["regressor_drops_a_shape_component"] = in_units(np.abs(blend_ref(m, 0, X, "regressor_drops_a_shape_component")[0] - bref), unit)
    bounds = {"pose_prepare": POSE_BOUND, "chain_trans": CHAIN_TRANS_BOUND, "chain_atrans": CHAIN_ATRANS_BOUND, "skin": SKIN_BOUND,
              "landmarks": LMK_BOUND, "blend": BLEND_BOUND}
    assert set(moved) == set(DEFECTS)
    for d, e in moved.items():
        b = bounds[DEFECTS[d]]
        assert math.isfinite(b), f"the {DEFECTS[d]} bound is not set"
        print(f"\n[defect] {d}: {e:.3e} = {e / b:.0f} x the {DEFECTS[d]} bound {b:.1e}")
        assert e >= 10 * b, f"{d} moves the result by {e:.2e} only, under 10x the {DEFECTS[d]} bound {b:.1e}"


def test_bounds_under_every_ceiling():
    for b, c in ((BLEND_BOUND, gemm_ceiling(512)), (CHAIN_ROT_BOUND, ROT_CEILING), (CHAIN_TRANS_BOUND, TRANS_CEILING),
                 (CHAIN_ATRANS_BOUND, ATRANS_CEILING), (SKIN_BOUND, skin_ceiling(1)), (LMK_BOUND, LMK_CEILING)):
        assert b <= c
    assert D_MAX == 10
