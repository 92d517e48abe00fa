"""BA windows of 57 to 128 optimised keyframes (visual, global) and 23 to 51 (inertial): the sizes at which the per-panel reduced solve
(ba_big_step_kernel per 16-column panel + ba_big_back_kernel, n > 320) first takes each of its strided, multi-pass and full-array paths.
Test infrastructure only (tests/test_ba_large_cpu.py proves the conditions on the cases; tests/test_ba_large_gpu.py runs them).

Visual and global windows come from covis_windows.covis_window (its corridor grows with K + F, so every keyframe of a 128-keyframe window
sees a stretch of it, and a dozen far points that every camera sees couple all keyframes: see _covis_with_common_points; synth.ba_window's cameras walk past one 12 m cloud and the late keyframes of a long window see nothing).  Global maps
have one fixed keyframe and some points behind the cameras that observe them, as tests/test_global_ba.py's _map.  Inertial windows are
synth.inertial_window's with a short keyframe interval, so that the last keyframe still sees the cloud, and FEW points: the inertial
oracle is dense in 15 K + 3 M unknowns.

paths(n, visual) restates from the constants of csrc/ba_kernels.hip which of those paths a reduced system of n unknowns reaches.
"""
import numpy as np

import orb_slam3_rust_amd as P
import covis_windows as W

synth = P.synth

# ---- the constants of orb-slam3-rust_amd/csrc/ba_kernels.hip, copied as numbers ---------------------------------------------------------
BF_MAX_N = 320              # "constexpr int BF_THREADS = 1024, BF_MAX_N = 320;": larger systems take one launch per panel
BA_MAX_N = 768              # "constexpr int BA_MAX_N = 768;"
BB_NB = 16                  # "constexpr int BB_NB = 16;": columns per panel
BB_STEP_THREADS = 512       # "#define ORBX_BB_STEP_THREADS 512"
BB_STEP_WAVES = 8           # "BB_STEP_WAVES = BB_STEP_THREADS / 64"
BB_COL_TILES = 6            # "BB_COL_TILES = (BA_MAX_N / 16 + BB_STEP_WAVES - 1) / BB_STEP_WAVES"
BACK_THREADS = 256          # "__launch_bounds__(256) void ba_big_back_kernel"
BACK_ROWS = 3               # "BACK_ROWS = (BA_MAX_N + 255) / 256" in ba_big_back_kernel
GATHER_MAX_BLOCKS = 2048    # "#define ORBX_BA_GATHER_MAX_BLOCKS 2048"
GATHER_LANES = 8            # "constexpr int BA_GATHER_LANES = 8;"
ASM_MAX_BLOCKS = 512        # "s.max_asm = std::max(s.max_asm, std::min(512, (pl.n * pl.n + 255) / 256));" in ba_launch_shape
SCHUR_BLOCK_COLS = 128      # "d.ncb = (d.ntile + 7) / 8;" in ba_plan_dims: 128-column blocks of the padded system
KSPLIT_MAX = 128            # "d.ksplit = std::max(1, std::min(128, (M + BA_PPS_TARGET - 1) / BA_PPS_TARGET));", 32 points per split

# every row of the table the cases must cover between them (tests/test_ba_large_cpu.py: test_cases_reach_every_path)
VISUAL_ROWS = ("gather_grid_capped", "assemble_second_pass", "schur_4_column_blocks", "schur_5_column_blocks", "schur_6_column_blocks",
               "column_tile_slot_3", "column_tile_slot_4", "column_tile_slot_5", "rows_below_second_pass", "rows_below_second_pass_is_rhs",
               "rhs_update_second_pass", "back_rows_q2", "full_768")
INERTIAL_ROWS = ("column_tile_slot_3", "column_tile_slot_4", "column_tile_slot_5", "rows_below_second_pass", "rhs_update_second_pass",
                 "back_rows_q2", "odd_stride_765")


def paths(n, visual):
    """The names of the paths that a reduced system of n unknowns reaches in the per-panel solve (an empty set where n <= BF_MAX_N: the
    one-launch factorisation).  visual: n = 6 K and the system comes from the Schur product, ba_gather_kernel and
    ba_big_assemble_kernel; otherwise n = 15 K, the inertial window's system, which its own kernel assembles (its visual part, 6 K <= 306,
    stays below every threshold of those three)."""
    assert 0 < n <= BA_MAX_N
    got = set()
    if n <= BF_MAX_N:
        return got
    got.add("per_panel")
    if visual:
        # ba_launch_shape: min(cap, ceil(lanes * n * ceil(n / 2) / 256)) blocks of 256 threads; at the cap the kernel's loop strides
        if (GATHER_LANES * n * ((n + 1) // 2) + 255) // 256 >= GATHER_MAX_BLOCKS:
            got.add("gather_grid_capped")
        # ba_big_assemble_kernel: "for (size_t idx = gt; idx < nn; idx += nth)" with nth = 256 * min(512, ceil(n n / 256))
        if n * n > 256 * ASM_MAX_BLOCKS:
            got.add("assemble_second_pass")
        padded = max(16, (n + 15) & ~15)                                    # "d.P = std::max(16, (6 * K + 15) & ~15);"
        ncb = (padded + SCHUR_BLOCK_COLS - 1) // SCHUR_BLOCK_COLS
        if ncb >= 4:
            got.add("schur_%d_column_blocks" % ncb)
    # the panel block, first launch with a previous panel (c0 = 16): nt = ceil((n - c0) / 16) tile rows, tile ti = wave + 8 t in slot t
    nt = (n - BB_NB + 15) // 16
    for t in range(3, BB_COL_TILES):
        if nt > BB_STEP_WAVES * t:
            got.add("column_tile_slot_%d" % t)
    # rows below the first panel and the right-hand side as row n: "for (int r = r0; r <= n; r += BB_STEP_THREADS)", r0 = 16 + tid
    if n - BB_NB + 1 > BB_STEP_THREADS:
        got.add("rows_below_second_pass")
        if n - BB_NB + 1 == BB_STEP_THREADS + 1:
            got.add("rows_below_second_pass_is_rhs")
    # "for (int r = c0 + tid; r < n; r += BB_STEP_THREADS)" at c0 = 16
    if n - BB_NB > BB_STEP_THREADS:
        got.add("rhs_update_second_pass")
    # ba_big_back_kernel: row i = tid + 256 q above the last panel (i < c_last)
    c_last = ((n - 1) // BB_NB) * BB_NB
    if c_last > BACK_THREADS * (BACK_ROWS - 1):
        got.add("back_rows_q2")
    if n == BA_MAX_N:
        got.add("full_768")
    if n == 15 * (BA_MAX_N // 15):
        got.add("odd_stride_765")
    return got


def slot_rows(n, t):
    """rows of the system that slot t of the panel block holds at the first panel that has a previous one (c0 = 16): tiles ti >= 8 t"""
    return max(0, n - (BB_NB + 16 * BB_STEP_WAVES * t))


def last_panel_width(n):
    """columns of the short last panel (0: full panels only)"""
    return n % BB_NB


# ---- the cases (seeds: tests/test_ba_large_cpu.py's docstring says how they were chosen and what they measure) -----------------------------
def _visual(seed, K, F):
    return dict(seed=seed, K=K, F=F, M=50 * K, step=1.0, keep=0.35, depth=(2, 6))


VISUAL = {                                                                 # K -> keyword arguments of covis_window
    57: _visual(2, 57, 12),
    61: _visual(1, 61, 17),
    65: _visual(2, 65, 10),
    67: _visual(1, 67, 14),
    87: _visual(1, 87, 19),
    88: _visual(1, 88, 11),
    89: _visual(3, 89, 16),
    109: _visual(1, 109, 13),
    110: _visual(1, 110, 20),
    128: _visual(1, 128, 15),
}
GLOBAL = {                                                                 # K optimised keyframes of a map of K + 1; (arguments, points behind the cameras)
    88: (dict(seed=1, K=88, F=1, M=4400, step=1.0, keep=0.35, depth=(2, 6)), 24),
    128: (dict(seed=1, K=128, F=1, M=6400, step=1.0, keep=0.35, depth=(2, 6)), 40),
}
INERTIAL = {                                                               # K -> (seed, M, dt): 15 K + 3 M <= 1300, a dense oracle solve of 1.5 - 2.3 s (tests/test_ba_large_cpu.py, which also says why 28 and 45)
    23: (3, 300, 0.08),
    27: (1, 290, 0.08),
    28: (3, 290, 0.08),
    35: (1, 250, 0.08),
    36: (1, 250, 0.08),
    44: (6, 210, 0.08),
    45: (1, 205, 0.08),
    51: (3, 175, 0.08),
}
COMMON_POINTS = 12                                                         # far points that every camera of a visual or global case observes
_cache = {}


def _covis_with_common_points(order, **kw):
    """covis_window's window plus COMMON_POINTS points far behind the middle of the corridor that EVERY camera observes.  The corridor alone
    gives a banded reduced system (keyframes far apart share no point) and a band stays a band under Cholesky: every tile more than a few
    keyframes from the diagonal — the Schur product's outer column-block pairs, the panel block's tile slots 3 to 5, the rows of the
    second passes — would hold exact zeros, and a kernel that dropped or misplaced them would give the same answer.  With these points
    every pair of keyframes is coupled and every tile of the system carries values.  (covis_window's own long_tracks option trims its
    tracks among the fixed cameras and needs about a hundred of them.)  They are the last COMMON_POINTS points of the window."""
    w = W.covis_window(order="kf_major", **kw)
    cam = w["camera"]; n = COMMON_POINTS; M = len(w["points"])
    rng = np.random.default_rng([0xC5, kw["seed"]])
    span = kw["step"] * (kw["K"] + kw["F"])
    z0 = 2.0 * (span / 2 + 1.0) * cam["fx"] / cam["cx"]                    # |x - camera x| <= span / 2 + 1 stays inside the image (covis_window: long_tracks)
    X = np.stack([span / 2 + rng.uniform(-1, 1, n), rng.uniform(-1.5, 1.5, n), rng.uniform(z0, z0 + 4.0, n)], 1)
    parts = [w["obs"]]
    for role, poses in (("f", w["fixed_cw"]), ("o", w["gt_poses_cw"])):
        for slot, pose in enumerate(poses):
            pc = synth._quat_rot(pose[:4], X) + pose[4:]
            u = cam["fx"] * pc[:, 0] / pc[:, 2] + cam["cx"]; v = cam["fy"] * pc[:, 1] / pc[:, 2] + cam["cy"]
            assert np.all((pc[:, 2] > 0.1) & (u >= 0) & (u < 752) & (v >= 0) & (v < 480)), "a camera does not see a common point"
            o = np.zeros(n, P.BA_OBS)
            o["kf_idx"] = slot if role == "o" else -1; o["fixed_idx"] = slot if role == "f" else -1
            o["mp_idx"] = M + np.arange(n); o["u"] = u + rng.normal(0, 1.0, n); o["v"] = v + rng.normal(0, 1.0, n)
            parts.append(o)
    w["obs"] = W.reorder(np.concatenate(parts), order, kw["seed"])
    w["points"] = np.concatenate([w["points"], X + rng.normal(0, 0.03, X.shape)])
    w["gt_points"] = np.concatenate([w["gt_points"], X])
    w["common"] = M + np.arange(n)
    return w


def visual_window(K, order="shuffled", seed=None):
    """the visual case of K optimised keyframes (made once per order and process; read-only).  seed: another seed of the same shape."""
    key = ("v", K, order, seed)
    if key not in _cache:
        kw = dict(VISUAL[K])
        if seed is not None:
            kw["seed"] = seed
        _cache[key] = _covis_with_common_points(order, **kw)
    return _cache[key]


def global_map(K, order="shuffled", seed=None):
    """the global case: one fixed keyframe, K optimised ones, and `behind` (indices) points that start behind the cameras that observe them — their
    observations keep the penalty and get no Jacobian, so the solver must hand them back untouched (tests/test_global_ba.py: _map)"""
    key = ("g", K, order, seed)
    if key not in _cache:
        kw, n_behind = GLOBAL[K]
        kw = dict(kw)
        if seed is not None:
            kw["seed"] = seed
        w = _covis_with_common_points(order, **kw)
        j = np.random.default_rng([0xC4, kw["seed"]]).permutation(kw["M"])[:n_behind]   # (none of the common points)
        w["points"] = w["points"].copy()
        w["points"][j, 2] = -w["points"][j, 2] - 5.0                        # the cameras look along +z from z ~ 0
        w["behind"] = j
        _cache[key] = w
    return _cache[key]


def inertial_window(K, seed=None):
    key = ("i", K, seed)
    if key not in _cache:
        s, M, dt = INERTIAL[K]
        _cache[key] = synth.inertial_window(s if seed is None else seed, K, M, P.BA_OBS, n_fixed=1, dt=dt)
    return _cache[key]


def kf_obs(window):
    """observations per optimised keyframe"""
    o = window["obs"]
    K = len(window["poses_cw"]) if "poses_cw" in window else len(window["poses_wc"])
    return np.bincount(o["kf_idx"][o["kf_idx"] >= 0], minlength=K)


# ---- the reference's answers, computed once per process and shared by the tests that compare with them -----------------------------------
_oracle_cache = {}


def _gcfg(oracle):
    return oracle.BaConfig(10, 1e-6, 1e-6, float(np.sqrt(5.991)), 0)        # tests/test_global_ba.py: _gcfg


def oracle_visual(oracle, K, order="shuffled", seed=None):
    key = ("v", K, order, seed)
    if key not in _oracle_cache:
        w = visual_window(K, order, seed)
        _oracle_cache[key] = oracle.ba_solve_schur(oracle.Camera(**w["camera"]), oracle.ba_config(), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    return _oracle_cache[key]


def oracle_global(oracle, K, order="shuffled", seed=None):
    key = ("g", K, order, seed)
    if key not in _oracle_cache:
        w = global_map(K, order, seed)
        _oracle_cache[key] = oracle.global_ba_solve_schur(oracle.Camera(**w["camera"]), _gcfg(oracle), w["poses_cw"], w["fixed_cw"], w["points"], w["obs"])
    return _oracle_cache[key]


def oracle_inertial(oracle, K, seed=None):
    key = ("i", K, seed)
    if key not in _oracle_cache:
        w = inertial_window(K, seed)
        _oracle_cache[key] = oracle.inertial_ba_solve(oracle.Camera(**w["camera"]), oracle.inertial_ba_config(), w["poses_wc"], w["velocities"], w["biases"],
                                                      w["fixed_cw"], w["points"], w["obs"], w["edge_kf"], w["preint"])
    return _oracle_cache[key]
