"""Float64 references, host models and case lists for the
first-generation HIP kernels (scans, projection, sum-tree, multi-tensor
polyak/RMSprop, Philox distributions, policy head, u8 dequantisation).

Shared by ``test_ops_reference_cpu.py`` (references against the fp32
CPU fallbacks, models against their invariants) and
``test_ops_edges_gpu.py`` (kernels against the references). Everything
here runs on the CPU: torch CPU tensors and numpy only.

Every reference is written from the formula in the ``machin_amd.ops``
docstrings and evaluates it in float64 over the *same fp32 input
values* the kernel sees; python scalars (``gamma``, ``v_min`` ...) are
first rounded to fp32, as the bindings do.

Error bounds. A scan reference returns, next to the float64 value, a
per-column magnitude ``M``: the same recurrence run over absolute
values, which bounds every intermediate the fp32 evaluation can form.
One fp32 rounding of an intermediate ``x`` costs at most
``2^-24 |x| <= 2^-24 M``, every recurrence here carries its error
forward with a factor ``<= 1``, so after ``T`` steps of ``c`` roundings
each ``|x - x64| <= c T 2^-24 M``. The ``C_*`` constants below are the
``c`` of each op, counted from the formula (one more than the count
where noted, for the second-order terms).
"""
import math

import numpy as np
import torch as t

U24 = 2.0 ** -24
# threads (or rows, or chunks) one pass of a capped grid covers: the
# kernels launch at most 2048 blocks of 256 threads and stride the rest
GRID_BLOCKS = 2048
GRID_THREADS = GRID_BLOCKS * 256


def f32(x) -> float:
    """The fp32 value of a python scalar, as a float64 python float."""
    return float(np.float32(x))


# ======================================================================
# scans
# ======================================================================
# (1,1): one thread; (7,65): past one wave; (3,257): past one block;
# (1000,3): long recurrence; the last has more columns than one pass of
# the grid, so the grid-stride loop runs a second time.
SCAN_SHAPES = [(1, 1), (7, 65), (3, 257), (1000, 3), (2, GRID_THREADS + 5)]
# n-step is one thread per (t, b) cell: T*B passes GRID_THREADS once in
# the last shape
NSTEP_SHAPES = [(1, 1), (7, 65), (40, 3), (5, GRID_THREADS // 5 + 7)]
SCAN_GAMMAS = [0.0, 1.0, 0.999]

# roundings per step, from the formulas in the ops docstrings
# R = r + (g*nd)*R: g*nd, *R, + r  -> 3 (+1 second order)
C_RETURNS = 4
# delta = r + (g*nd)*nv - v: 4; A = delta + ((g*lam)*nd)*A: 4 -> 8 (+1)
C_GAE = 9
# n-step term k: gamma^k carries k-1 roundings, *a, *r: <= m+1 per term
# and m additions, m = min(n, T) terms -> < 3 per term (+1)
C_NSTEP = 4
# vs: td 4, *rho 1, carry 4, + V 1 = 10 per step; pg_adv adds its own 4
# roundings on top of the error of vs[t+1], folded in as 4 more per step
C_VTRACE = 14


def scan_id(shape):
    return "x".join(str(s) for s in shape)


def make_scan_case(shape, seed=0, terminals="random"):
    """fp32 CPU inputs of every scan for ``[T, B]``; values of both
    signs, a few exact zeros, rewards up to a few units."""
    T, B = shape
    g = t.Generator().manual_seed(1000 + seed)
    rnd = lambda *s: t.randn(*s, generator=g)  # noqa: E731
    if terminals == "random":
        term = (t.rand(T, B, generator=g) < 0.15).float()
    elif terminals == "all":
        term = t.ones(T, B)
    else:
        term = t.zeros(T, B)
    rew = rnd(T, B) * 2
    rew[0, 0] = 0.0
    return {
        "rew": rew,
        "val": rnd(T, B) * 3,
        "next_val": rnd(T, B) * 3,
        "boot": rnd(B) * 3,
        "term": term,
    }


def make_vtrace_case(shape, seed=0, clipped=True, terminals="random"):
    """V-trace inputs. ``clipped``: ``tlp - blp >= 0.1`` everywhere, so
    every ratio is above every clip used (<= 1.05 < e^0.1) and the
    exponential cannot matter. Otherwise ``tlp - blp`` spans
    ``[-6, 0.5]`` and most ratios are used unclipped."""
    T, B = shape
    case = make_scan_case(shape, seed + 77, terminals)
    g = t.Generator().manual_seed(2000 + seed)
    blp = -t.rand(T, B, generator=g) * 3 - 0.05
    if clipped:
        diff = 0.1 + t.rand(T, B, generator=g) * 2
    else:
        diff = -6 + 6.5 * t.rand(T, B, generator=g)
    tlp = blp + diff
    # the sum is rounded: restore the floor exactly where it was lost
    if clipped:
        bad = (tlp - blp) < 0.1
        tlp = t.where(bad, blp + 0.2, tlp)
        assert bool(((tlp - blp) >= 0.1).all())
    case["blp"], case["tlp"] = blp, tlp
    return case


# clips of the tight case: distinct, so a swapped clip shows, and all
# below e^0.1 = 1.105
VTRACE_CLIPS_TIGHT = dict(rho_clip=1.0, c_clip=0.9, pg_rho_clip=1.05)
VTRACE_CLIPS_LOOSE = dict(rho_clip=1.0, c_clip=1.0, pg_rho_clip=1.0)


def ref_discounted_returns(rew, term, gamma, boot=None):
    """R_t = r_t + gamma (1 - d_t) R_{t+1}, R_T = bootstrap.
    Returns (R [T, B] float64, M [B])."""
    g = f32(gamma)
    r, nd = rew.double(), 1.0 - term.double()
    T, B = r.shape
    run = t.zeros(B, dtype=t.float64) if boot is None else boot.double().clone()
    mag = run.abs()
    out, M = t.empty_like(r), mag.clone()
    for i in range(T - 1, -1, -1):
        run = r[i] + g * nd[i] * run
        mag = r[i].abs() + g * nd[i] * mag
        out[i] = run
        M = t.maximum(M, mag)
    return out, M


def ref_gae(rew, val, next_val, term, gamma, lam):
    """A_t = delta_t + gamma lam (1 - d_t) A_{t+1},
    delta_t = r_t + gamma (1 - d_t) V_{t+1} - V_t."""
    g, la = f32(gamma), f32(lam)
    r, v, nv = rew.double(), val.double(), next_val.double()
    nd = 1.0 - term.double()
    T, B = r.shape
    run = t.zeros(B, dtype=t.float64)
    mag = run.clone()
    out, M = t.empty_like(r), mag.clone()
    for i in range(T - 1, -1, -1):
        run = (r[i] + g * nd[i] * nv[i] - v[i]) + g * la * nd[i] * run
        mag = (r[i].abs() + g * nd[i] * nv[i].abs() + v[i].abs()
               + g * la * nd[i] * mag)
        out[i] = run
        M = t.maximum(M, mag)
    return out, M


def ref_nstep_returns(rew, term, gamma, n):
    """G_t = sum_{k<n, t+k<T} gamma^k r_{t+k} prod_{j<k} (1 - d_{t+j}).
    Returns (G [T, B] float64, M [T, B])."""
    g = f32(gamma)
    r, alive = rew.double(), 1.0 - term.double()
    T, B = r.shape
    out, M = t.zeros_like(r), t.zeros_like(r)
    a = t.ones_like(r)  # a[t] = prod_{j<k} alive[t+j]
    for k in range(min(max(1, int(n)), T)):
        rows = T - k
        out[:rows] += (g ** k) * a[:rows] * r[k:]
        M[:rows] += (g ** k) * a[:rows] * r[k:].abs()
        a[:rows] = a[:rows] * alive[k:]
    return out, M


def ref_vtrace(blp, tlp, rew, val, boot, term, gamma, rho_clip=1.0,
               c_clip=1.0, pg_rho_clip=1.0):
    """IMPALA V-trace, time-major ``[T, B]``:
    rho = exp(tlp - blp),
    vs_t - V_t = min(rho, rho_clip) (r + g nd V_{t+1} - V_t)
                 + g nd min(rho, c_clip) (vs_{t+1} - V_{t+1}),
    pg_t = min(rho, pg_rho_clip) (r + g nd vs_{t+1} - V_t),
    V_T = vs_T = bootstrap. Returns (vs, pg, M [B])."""
    g = f32(gamma)
    rc, cc, pc = f32(rho_clip), f32(c_clip), f32(pg_rho_clip)
    r, v, nd = rew.double(), val.double(), 1.0 - term.double()
    rho = t.exp(tlp.double() - blp.double())
    T, B = r.shape
    b = boot.double().view(B)
    acc = t.zeros(B, dtype=t.float64)
    macc = acc.clone()
    vs_next, v_next = b.clone(), b.clone()
    mvs_next = b.abs()
    vs, pg = t.empty_like(r), t.empty_like(r)
    M = b.abs()
    for i in range(T - 1, -1, -1):
        c_rho = rho[i].clamp(max=rc)
        td = r[i] + g * nd[i] * v_next - v[i]
        mtd = r[i].abs() + g * nd[i] * v_next.abs() + v[i].abs()
        acc = c_rho * td + g * nd[i] * rho[i].clamp(max=cc) * acc
        macc = c_rho * mtd + g * nd[i] * rho[i].clamp(max=cc) * macc
        p_rho = rho[i].clamp(max=pc)
        pg[i] = p_rho * (r[i] + g * nd[i] * vs_next - v[i])
        mpg = p_rho * (r[i].abs() + g * nd[i] * mvs_next + v[i].abs())
        vs[i] = acc + v[i]
        mvs = macc + v[i].abs()
        M = t.maximum(M, t.maximum(mvs, mpg))
        vs_next, v_next, mvs_next = vs[i], v[i], mvs
    return vs, pg, M


def scan_bound(c, steps, M):
    """``c steps 2^-24 M``, broadcast over the time axis for [B]."""
    return c * steps * U24 * M


# ======================================================================
# categorical projection
# ======================================================================
PROJ_RANGES = [(-10.0, 10.0), (0.0, 1.0), (-1.0, 1.0), (0.0, 200.0),
               (-5.0, 5.0)]
PROJ_ATOMS = range(2, 257)
PROJ_RTOL, PROJ_ATOL = 1e-4, 1e-3  # the project's projection tolerance
PROJ_MASS_TOL = 1e-5
# more rows than one pass of the grid: 2048 blocks of 4 row-waves
PROJ_BATCHES = [1, 5, GRID_BLOCKS * 4 + 8]


def projection_overshoots(v_min, v_max, atoms) -> bool:
    """Whether the fp32 formula ``(v_max - v_min) / delta_z`` lands
    above the last bin ``atoms - 1``."""
    lo, hi = np.float32(v_min), np.float32(v_max)
    delta_z = (hi - lo) / np.float32(atoms - 1)
    pos = (hi - lo) / delta_z
    assert pos.dtype == np.float32
    return bool(pos > np.float32(atoms - 1))


def overshooting_supports():
    """Every ``(v_min, v_max, atoms)`` of the enumeration whose fp32
    position of ``v_max`` overshoots the support."""
    return [
        (lo, hi, a) for lo, hi in PROJ_RANGES for a in PROJ_ATOMS
        if projection_overshoots(lo, hi, a)
    ]


def make_projection_case(batch, atoms, v_min, v_max, seed=0):
    """fp32 CPU ``(dist, rew, term)``. Rows, where the batch has them:
    last: every atom clamped to ``v_max``; 0: clamped to ``v_min``;
    1: terminal with the reward exactly on the top atom; 2: terminal on
    the bottom atom; 3: terminal near a middle atom; the rest random,
    one in five terminal."""
    g = t.Generator().manual_seed(3000 + seed + 7 * atoms + batch)
    span = v_max - v_min
    dist = t.softmax(
        t.randn(batch, atoms, generator=g, dtype=t.float64) * 2, dim=1
    ).float()
    rew = (v_min + span * (t.rand(batch, generator=g) * 1.2 - 0.1)).float()
    term = (t.rand(batch, generator=g) < 0.2).float()
    if batch > 1:
        rew[0], term[0] = v_min - 2 * span, 0.0
    if batch > 2:
        rew[1], term[1] = v_max, 1.0
    if batch > 3:
        rew[2], term[2] = v_min, 1.0
    if batch > 4:
        rew[3] = v_min + span * (atoms // 2) / (atoms - 1)
        term[3] = 1.0
    rew[batch - 1], term[batch - 1] = v_max + 2 * span, 0.0
    return dist, rew, term


def ref_projection(dist, rew, term, gamma, v_min, v_max):
    """Project ``r + gamma (1 - d) z`` onto the support in float64.
    The position is ``(tz - v_min) (A - 1) / (v_max - v_min)``, which
    is exactly ``A - 1`` at ``tz == v_max``: it never leaves
    ``[0, A - 1]``."""
    B, A = dist.shape
    g, lo_v, hi_v = f32(gamma), f32(v_min), f32(v_max)
    p = dist.double()
    r = rew.double().view(B, 1)
    nd = 1.0 - term.double().view(B, 1)
    z = lo_v + (hi_v - lo_v) * t.arange(A, dtype=t.float64) / (A - 1)
    tz = (r + g * nd * z.view(1, A)).clamp(lo_v, hi_v)
    pos = (tz - lo_v) * (A - 1) / (hi_v - lo_v)
    assert float(pos.min()) >= 0.0 and float(pos.max()) <= A - 1
    lo_f, hi_f = pos.floor(), pos.ceil()
    w_lo = t.where(lo_f == hi_f, t.ones_like(pos), hi_f - pos)
    w_hi = pos - lo_f
    proj = t.zeros_like(p)
    proj.scatter_add_(1, lo_f.long(), p * w_lo)
    proj.scatter_add_(1, hi_f.long(), p * w_hi)
    return proj


# ======================================================================
# Philox4x32-10 and the kernels' normal
# ======================================================================
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)

# (counter, key, output): the published known-answer vectors
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0),
     (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds (Salmon et al. 2011). ``ctr``: four
    and ``key``: two arrays (or ints) of 32-bit values; returns four
    uint64 arrays holding 32-bit values."""
    c = [np.atleast_1d(np.asarray(x, dtype=np.uint64)) for x in ctr]
    k0, k1 = (np.asarray(x, dtype=np.uint64) for x in key)
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]  # 32x32 -> 64 bits, no overflow
        c = [
            (p1 >> _S32) ^ c[1] ^ k0,
            p1 & _MASK,
            (p0 >> _S32) ^ c[3] ^ k1,
            p0 & _MASK,
        ]
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c


def philox_uniform(x):
    """The kernels' map of 32 random bits to (0, 1]:
    ``(x >> 8) 2^-24 + 2^-25`` evaluated in fp32 as the kernel does
    (the sum needs 25 bits, so it is rounded), returned as float64."""
    hi = (np.asarray(x, dtype=np.uint64) >> np.uint64(8)).astype(np.float32)
    u = hi * np.float32(2.0 ** -24) + np.float32(2.0 ** -25)
    assert u.dtype == np.float32
    return u.astype(np.float64)


def philox_normal(seed, offset, index):
    """The standard normal the kernels draw for flat element ``index``:
    key = seed (low, high), ctr = (offset low, offset high, index low,
    index high), Box-Muller in float64 over the first two outputs, the
    first (cosine) normal."""
    seed, offset = int(seed), int(offset)
    idx = np.asarray(index, dtype=np.uint64)
    shape = idx.shape
    idx = idx.reshape(-1)
    full = np.full_like(idx, 1)
    r = philox4x32_10(
        (full * np.uint64(offset & 0xFFFFFFFF),
         full * np.uint64(offset >> 32),
         idx & _MASK, idx >> _S32),
        (seed & 0xFFFFFFFF, seed >> 32),
    )
    u1, u2 = philox_uniform(r[0]), philox_uniform(r[1])
    n = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
    return n.reshape(shape)


# ======================================================================
# Gaussian log-probabilities
# ======================================================================
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
GAUSS_SHAPES = [(1, 1), (5, 65), (GRID_BLOCKS * 4 + 8, 3)]
# roundings of one element's term in fp32: u or act (2), z (3), the
# term's three subtractions (3)
C_GAUSS = 8


def ref_gaussian_logprob(mu, log_std, act, tanh_squash=False,
                         epsilon=1e-6):
    """log N(u; mu, exp(log_std)) summed over the last axis, with
    ``u = act`` or, squashed, ``u = atanh(c)``,
    ``c = clamp(act, -(1 - 1e-6), 1 - 1e-6)`` (the fp32 constant) and
    the correction ``- log(1 - c^2 + epsilon)``.

    Returns ``(logp [B, 1] float64, bound [B, 1])``. The bound is what
    an fp32 evaluation of the formula may differ by: per element
    ``C_GAUSS 2^-24`` of the magnitudes the term is built from, the
    rounding of ``u`` carried through ``z^2`` and, squashed, the
    cancellation in ``1 - c^2 + epsilon`` (``c^2`` is rounded at
    ``2^-25`` absolute, which the small sum divides)."""
    m, ls, a = mu.double(), log_std.double(), act.double()
    inv_std = t.exp(-ls)
    eps_c = f32(epsilon)
    if tanh_squash:
        lim = float(np.float32(1.0) - np.float32(1e-6))
        c = a.clamp(-lim, lim)
        lp, lm = t.log1p(c), t.log1p(-c)
        u = 0.5 * (lp - lm)
        s = 1.0 - c * c + eps_c
        sq = t.log(s)
        du = U24 * (2.0 + 2.0 * lp.abs() + 2.0 * lm.abs())
        dsq = U24 * (c * c + 2.0 * s) / s + 2.0 * U24 * sq.abs()
    else:
        u, sq = a, t.zeros_like(a)
        du, dsq = t.zeros_like(a), t.zeros_like(a)
    z = (u - m) * inv_std
    term = -0.5 * z * z - ls - LOG_SQRT_2PI - sq
    dz = (du + 2.0 * U24 * (u.abs() + m.abs())) * inv_std \
        + 4.0 * U24 * z.abs()
    mags = 0.5 * z * z + ls.abs() + LOG_SQRT_2PI + sq.abs()
    D = a.shape[1]
    per = z.abs() * dz + dsq + C_GAUSS * U24 * mags
    bound = per.sum(dim=1, keepdim=True) \
        + (7 + D // 64) * U24 * mags.sum(dim=1, keepdim=True)
    return term.sum(dim=1, keepdim=True), bound


def make_gauss_case(shape, seed=0):
    B, D = shape
    g = t.Generator().manual_seed(4000 + seed)
    mu = t.randn(B, D, generator=g)
    log_std = t.rand(B, D, generator=g) * 1.5 - 1.0  # [-1, 0.5]
    return mu, log_std


# ======================================================================
# sum-tree
# ======================================================================
# below, at and above the 4096-node LDS stage; non-powers of two
SUMTREE_SIZES = [1, 2, 5, 1000, 4096, 5000, 100000]
SUMTREE_FILLS = ["full", "37", "60%"]


def sumtree_cases():
    out = []
    for size in SUMTREE_SIZES:
        for fill in SUMTREE_FILLS:
            if fill == "37" and size < 37:
                continue
            out.append((size, fill))
    return out


def make_leaf_weights(size, fill, seed=0):
    """fp32 leaf weights [size]: ``rand**4 + 1e-3`` on the filled
    prefix, a tenth of it (leaf 0 included) zeroed, the rest never
    written (zero)."""
    rng = np.random.RandomState(5000 + seed + size)
    filled = {"full": size, "37": 37,
              "60%": int(math.ceil(0.6 * size))}[fill]
    w = np.zeros(size, dtype=np.float32)
    w[:filled] = (rng.rand(filled) ** 4 + 1e-3).astype(np.float32)
    if filled >= 2:
        k = max(1, filled // 10)
        dead = rng.choice(np.arange(1, filled), size=k - 1, replace=False) \
            if k > 1 else np.zeros(0, dtype=np.int64)
        w[dead] = 0.0
        w[0] = 0.0
    return w


def make_update_rounds(size, seed=0):
    """Three ``(weights, indexes)`` rounds: distinct indexes with a few
    zero weights; duplicate indexes carrying equal weights; length 1."""
    rng = np.random.RandomState(6000 + seed + size)
    k = max(1, min(size, 300) // 2)
    idx_a = rng.choice(size, size=k, replace=False).astype(np.int64)
    w_a = (rng.rand(k) ** 4 + 1e-3).astype(np.float32)
    w_a[::7] = 0.0
    if size > 1:
        # never leave the tree without weight
        w_a[0] = 0.5
    base = rng.choice(size, size=max(1, k // 2), replace=True).astype(np.int64)
    idx_b = np.concatenate([base, base[::-1], base[:1]])
    per_leaf = (rng.rand(size) + 0.25).astype(np.float32)
    w_b = per_leaf[idx_b]
    idx_c = np.array([size - 1], dtype=np.int64)
    w_c = np.array([0.75], dtype=np.float32)
    return [(w_a, idx_a), (w_b, idx_b), (w_c, idx_c)]


def rule_guarded(w, lw, rw):
    """The walk of ``DeviceSumTree.find_leaf_index``: right iff the
    right subtree holds weight and ``w > lw`` or the left one is
    empty; a tie stays left."""
    return (rw > 0) & ((w > lw) | ~(lw > 0))


def rule_unguarded(w, lw, rw):
    """The walk without the zero-subtree guard (never looks right)."""
    return w > lw


def sumtree_walk(nodes, u, capacity, depth, size, rule=rule_guarded):
    """fp32 model of the root-to-leaf walk over the node array
    ``nodes [2 capacity]``; returns int64 leaf indexes."""
    nodes = np.asarray(nodes, dtype=np.float32)
    w = np.asarray(u, dtype=np.float32).copy()
    node = np.ones(w.shape, dtype=np.int64)
    for _ in range(depth):
        left = node << 1
        lw, rw = nodes[left], nodes[left + 1]
        right = rule(w, lw, rw)
        w = np.where(right, w - lw, w).astype(np.float32)
        node = left + right
    return np.clip(node - capacity, 0, size - 1)


def sumtree_queries(nodes, capacity, size, seed=0):
    """fp32 queries in the closed range ``[0, total]``: 4096 stratified
    ones as ``DeviceSumTree.sample`` forms them, both ends, the last
    fp32 value below the total and every leaf's fp32 prefix
    boundary."""
    nodes = np.asarray(nodes, dtype=np.float32)
    total = nodes[1]
    rng = np.random.RandomState(7000 + seed + size)
    n = 4096
    strat = (rng.rand(n).astype(np.float32)
             + np.arange(n, dtype=np.float32)) * (total / np.float32(n))
    leaves = nodes[capacity:capacity + size]
    bounds = np.cumsum(leaves, dtype=np.float32)
    ends = np.array(
        [0.0, total, np.nextafter(total, np.float32(0.0))], dtype=np.float32
    )
    u = np.concatenate([strat.astype(np.float32), ends, bounds])
    return np.clip(u, np.float32(0.0), total).astype(np.float32)


def check_tree_nodes(nodes, capacity, size, leaves):
    """Node-array invariants: written leaves read back exactly, padding
    leaves are zero, every internal node is the fp32 sum of its two
    children exactly."""
    nodes = np.asarray(nodes)
    assert nodes.dtype == np.float32 and nodes.shape == (2 * capacity,)
    assert np.array_equal(nodes[capacity:capacity + size], leaves)
    assert not nodes[capacity + size:].any()
    want = nodes[2:2 * capacity:2] + nodes[3:2 * capacity:2]
    assert want.dtype == np.float32
    bad = np.nonzero(nodes[1:capacity] != want)[0]
    assert bad.size == 0, f"nodes {bad[:5] + 1} are not their children's sum"


def check_leaves_found(nodes, capacity, depth, size, u, leaf):
    """What a returned leaf must satisfy for query ``u``: it has weight,
    and against the float64 prefix sums ``c`` of the leaves
    ``c[i-1] - s <= u <= c[i] + s`` with ``s = depth 2^-23 total``
    (the rounding of the node sums and subtractions along one path)."""
    nodes = np.asarray(nodes, dtype=np.float32)
    leaves = nodes[capacity:capacity + size].astype(np.float64)
    leaf = np.asarray(leaf)
    assert leaf.min() >= 0 and leaf.max() < size
    dead = np.nonzero(leaves[leaf] <= 0)[0]
    assert dead.size == 0, (
        f"{dead.size} queries returned a zero-weight leaf, e.g. "
        f"u={u[dead[:3]]} -> leaf {leaf[dead[:3]]}"
    )
    c = np.cumsum(leaves)
    s = depth * 2.0 ** -23 * float(nodes[1])
    upper = c[leaf]
    lower = np.where(leaf > 0, c[np.maximum(leaf - 1, 0)], 0.0)
    u64 = np.asarray(u, dtype=np.float64)
    bad = np.nonzero((u64 < lower - s) | (u64 > upper + s))[0]
    assert bad.size == 0, (
        f"{bad.size} leaves outside their prefix interval, e.g. "
        f"u={u64[bad[:3]]} -> leaf {leaf[bad[:3]]}"
    )


# ======================================================================
# multi-tensor polyak and RMSprop
# ======================================================================
MT_CHUNK = 4096
# tensor boundaries inside chunks, on a chunk edge, an empty tensor
MT_NUMELS = [1, 4095, 4096, 4097, 0, 37, 3 * 4096 + 1]
MT_MANY = [1] * 300
# one tensor past a whole pass of the grid (2048 chunks)
MT_LONG = [GRID_BLOCKS * MT_CHUNK + 4099]
MT_LISTS = {"edges": MT_NUMELS, "many": MT_MANY, "long": MT_LONG}
POLYAK_TAUS = [0.0, 1.0, 0.005]


def make_polyak_case(numels, seed=0):
    """Positive fp32 ``(targets, sources)`` in [0.5, 1.5): with no
    cancellation between the two products, an fp32 evaluation (fused
    or not) stays within one ulp of the rounded float64 result."""
    g = t.Generator().manual_seed(8000 + seed)
    tgt = [t.rand(n, generator=g) + 0.5 for n in numels]
    src = [t.rand(n, generator=g) + 0.5 for n in numels]
    return tgt, src


def make_polyak_mixed_case(numels, seed=0):
    """fp32 ``(targets, sources)`` of both signs and a wide range of
    magnitudes, zeros included: the two products cancel in places."""
    g = t.Generator().manual_seed(8500 + seed)

    def draw(n):
        x = t.randn(n, generator=g) * t.exp(t.randn(n, generator=g) * 3)
        x[::11] = 0.0
        return x

    return [draw(n) for n in numels], [draw(n) for n in numels]


def polyak_mixed_ok(got, tgt0, src0, tau):
    """``|got - (keep t + tau s)| <= 2^-23 (|keep t| + |tau s|)``
    against float64: an unfused fp32 evaluation rounds both products
    and the sum, half an ulp (<= 2^-24 relative) each, and the sum is
    no larger than the two products together; a fused one does less."""
    tau32 = np.float32(tau)
    keep = float(np.float32(1.0) - tau32)
    a = keep * tgt0.double()
    b = float(tau32) * src0.double()
    err = (got.double() - (a + b)).abs()
    return bool((err <= 2.0 ** -23 * (a.abs() + b.abs())).all())


def ref_polyak(tgt, src, tau):
    """``keep t + tau s`` in float64 over the fp32 ``tau`` and
    ``keep = 1 - tau`` (an fp32 subtraction), rounded to fp32."""
    tau32 = np.float32(tau)
    keep = float(np.float32(1.0) - tau32)
    return [
        (keep * a.double() + float(tau32) * b.double()).float()
        for a, b in zip(tgt, src)
    ]


def ulp_distance_ok(got, want):
    """Elementwise ``|got - want| <= 1 ulp`` of the larger magnitude."""
    g, w = got.numpy(), want.numpy()
    ulp = np.spacing(np.maximum(np.abs(g), np.abs(w)).astype(np.float32))
    return bool((np.abs(g.astype(np.float64) - w) <= ulp).all())


# alpha = 127/128 is exact in fp32, so is 1 - alpha: the eager chain
# (which rounds the double 1 - alpha) and an fp32 kernel (which
# subtracts the rounded alpha) then share their constants, and the
# measured allowance is about arithmetic only. With alpha = 0.99 the
# two constants differ by 1e-6 relative.
RMS_HYPER = dict(lr=1e-2, alpha=0.9921875, eps=1e-2)
RMS_STEPS = 3
# max_norm <= 0: no clipping, the norm pass is skipped; 0.5: engaged
# (the gradient norm is in the hundreds); 1e6: computed, not engaged
RMS_MAX_NORMS = {"skip": 0.0, "clip": 0.5, "noclip": 1e6}


def make_rmsprop_case(numels, seed=0):
    """fp32 ``(params, square_avg, [grads per step])``."""
    g = t.Generator().manual_seed(9000 + seed)
    params = [t.randn(n, generator=g) for n in numels]
    sq = [t.rand(n, generator=g) * 0.5 for n in numels]
    grads = [
        [t.randn(n, generator=g) * (1.0 + k) for n in numels]
        for k in range(RMS_STEPS)
    ]
    return params, sq, grads


def ref_rmsprop(params, sq, grads, max_norm, lr, alpha, eps):
    """``clip_grad_norm_(max_norm)`` then RMSprop (momentum 0, not
    centered, no weight decay) in float64, ``len(grads)`` steps:
    scale = min(1, max_norm / (norm + 1e-6)) (1 if max_norm <= 0),
    g' = g scale, sq = alpha sq + (1 - alpha) g'^2,
    p -= lr g' / (sqrt(sq) + eps)."""
    lr, alpha, eps = f32(lr), f32(alpha), f32(eps)
    p = [x.double().clone() for x in params]
    s = [x.double().clone() for x in sq]
    for step in grads:
        gs = [x.double() for x in step]
        scale = 1.0
        if max_norm > 0:
            norm = math.sqrt(sum(float((x * x).sum()) for x in gs))
            scale = min(1.0, f32(max_norm) / (norm + f32(1e-6)))
        for i, gi in enumerate(gs):
            gi = gi * scale
            s[i] = alpha * s[i] + (1.0 - alpha) * gi * gi
            p[i] = p[i] - lr * gi / (s[i].sqrt() + eps)
    return p, s


def eager_rmsprop(params, sq, grads, max_norm, device="cpu", **hyper):
    """The eager fp32 chain on ``device``: returns ``(optimizer,
    parameter list)`` after a zero-gradient step that materialises the
    state (it changes nothing: g = 0 leaves sq at 0 and p in place)
    with ``square_avg`` then set to ``sq``; the caller steps."""
    ps = [t.nn.Parameter(x.clone().to(device)) for x in params]
    opt = t.optim.RMSprop(ps, **hyper)
    for p in ps:
        p.grad = t.zeros_like(p)
    opt.step()
    for p, x, s0 in zip(ps, params, sq):
        assert t.equal(p.detach().cpu(), x)
        opt.state[p]["square_avg"].copy_(s0)
    return opt, ps


def run_eager_rmsprop(params, sq, grads, max_norm, **hyper):
    """fp32 ``clip_grad_norm_`` + ``torch.optim.RMSprop`` on the CPU
    over all of ``grads``: ``(params, square_avg)`` lists."""
    opt, ps = eager_rmsprop(params, sq, grads, max_norm, **hyper)
    for step in grads:
        for p, g in zip(ps, step):
            p.grad.copy_(g)
        if max_norm > 0:
            t.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
    return ([p.detach() for p in ps],
            [opt.state[p]["square_avg"] for p in ps])


def max_abs_err(got, want64):
    """Largest elementwise error of a tensor list against float64."""
    worst = 0.0
    for g, w in zip(got, want64):
        if g.numel():
            worst = max(worst, float((g.detach().cpu().double() - w)
                                     .abs().max()))
    return worst


# ======================================================================
# categorical policy head
# ======================================================================
PG_ACTIONS = [1, 6, 32]
PG_ROWS = [1, 300, GRID_THREADS + 1]
# backward: one bf16 ulp of the float64 gradient rounded to bf16, as the
# C51 tests assert it
PG_BF16_RTOL = 2.0 ** -7
PG_BF16_ATOL = 1e-6


def pg_forward_bounds(actions, taken64, ent64):
    """What an fp32 log-softmax over ``A`` bf16 logits may differ from
    float64 by, each operation counted at one fp32 ulp (2^-23; libm's
    exp and log are good to an ulp, not half). ``x - max`` is exact.
    The sum of ``A`` exponentials carries ``A + 1`` ulps relative,
    which its logarithm turns into as many absolute; the logarithm and
    the final subtraction add ulps of ``|logsum| <= 1 + |logp|`` and of
    ``|logp|``: ``(A + 4) 2^-23 (1 + |logp|)`` for a log-probability.
    The entropy ``-sum p logp`` adds the error of ``p`` (as many ulps
    again, relative) and its own ``A`` additions:
    ``(3 A + 12) 2^-23 sum_a p (1 + |logp|) = (3 A + 12) 2^-23 (1 + H)``.
    Returns ``(taken bound [N], entropy bound [N])``."""
    ulp = 2.0 ** -23
    return ((actions + 4) * ulp * (1.0 + taken64.abs()),
            (3 * actions + 12) * ulp * (1.0 + ent64))


def make_pg_case(rows, actions, seed=0):
    """bf16 logits [rows, actions] (random within +-3; row 0 all equal,
    row 1 one value at +80, row 2 one at -80, where the batch has
    them), int64 actions, fp32 upstream gradients."""
    g = t.Generator().manual_seed(10000 + seed + rows + actions)
    logits = (t.randn(rows, actions, generator=g) * 1.5).clamp(-3, 3)
    logits[0] = 0.75
    if rows > 1:
        logits[1, actions // 2] = 80.0
    if rows > 2:
        logits[2, actions - 1] = -80.0
    act = t.randint(0, actions, (rows,), generator=g)
    if rows > 1:
        act[1] = actions // 2  # the certain action: 1 - p cancels
    return (logits.to(t.bfloat16), act,
            t.randn(rows, generator=g), t.randn(rows, generator=g))


def ref_pg_head(logits, act, g_taken, g_ent):
    """Float64 on the bf16 values: ``(taken log-prob, entropy,
    d logits)`` with
    d logits = g_taken (1[a == a_i] - p) - g_ent p (log p + H)."""
    x = logits.double()
    logp = t.log_softmax(x, dim=-1)
    p = logp.exp()
    ent = -(p * logp).sum(dim=-1)
    idx = act.view(-1, 1)
    taken = logp.gather(1, idx).view(-1)
    onehot = t.zeros_like(p).scatter_(1, idx, 1.0)
    gt = g_taken.double().view(-1, 1)
    ge = g_ent.double().view(-1, 1)
    H = ent.view(-1, 1)
    grad = gt * (onehot - p) - ge * p * (logp + H)
    return taken, ent, grad


# ======================================================================
# u8 dequantisation
# ======================================================================
# nothing, scalar tail only, below/at/above one 16-byte vector, and
# more vectors than one pass of the grid plus a tail
DEQUANT_SIZES = [0, 1, 15, 16, 17, 16 * GRID_THREADS + 9]
DEQUANT_SCALES = [1.0 / 255.0, 1.0]
