"""GPU tests of the first-generation gfx950 kernels (scans, projection,
sum-tree, multi-tensor polyak/RMSprop, Philox distributions, policy
head, u8 dequantisation) against the float64 references and host
models of ``util_ops_reference``, at the shapes where the launch
geometry changes: one thread, past one wave, past one block, past one
pass of the capped grid, tensor boundaries inside a chunk.

Tolerances.

* Returns, GAE, n-step and the fully clipped V-trace case: the derived
  worst-case bound ``c T 2^-24 M`` (``util_ops_reference``).
* Unclipped V-trace (``tlp - blp`` in [-6, 0.5]) and fused RMSprop:
  measured. The fp32 CPU chain's largest error against float64 is
  taken in the test, the kernel may have 8 times that (fast ``exp``,
  FMA contraction and, for RMSprop, the order of the atomic sum of
  squares are legitimate). Figures measured on an MI355X are listed in
  ``MEASURED`` below.
* Philox normals: the kernel's ``logf``/``sqrtf``/``__sincosf``
  Box-Muller against float64 over the same uniforms; the largest
  deviation over the (8200, 3) case was measured once
  (``NOISE_DEV_MEASURED``) and 4 times that is asserted everywhere.
  Above ``1e-3`` it would be a defect, not a tolerance.
* Projection: ``rtol=1e-4, atol=1e-3`` (the project's projection
  tolerance), mass conserved within ``1e-5`` per row.
* Polyak: within one ulp of the float64 result rounded to fp32.
* Policy head: forward within the derived fp32 bound
  (``pg_forward_bounds``) of float64 on the bf16 values, backward
  within one bf16 ulp (``rtol=2^-7, atol=1e-6``) of the float64
  gradient rounded to bf16.
* Sum-tree and dequantisation: exact.

MEASURED on an MI355X (largest error against float64: fp32 CPU chain /
kernel; the kernel is allowed 8 times the first figure):

* V-trace unclipped (7, 65): vs 7.19e-07 / 5.78e-07,
  pg_adv 6.87e-07 / 7.46e-07
* V-trace unclipped (1000, 3): vs 1.75e-06 / 1.75e-06,
  pg_adv 1.34e-06 / 1.05e-06
* RMSprop edges, no clipping (``max_norm`` 0 and 1e6):
  params 3.25e-07 / 3.25e-07, square_avg 1.05e-07 / 1.11e-07
* RMSprop edges, clipping engaged: params 3.10e-07 / 3.10e-07,
  square_avg 8.06e-08 / 8.06e-08
* RMSprop long, clipping engaged: params 6.63e-07 / 6.63e-07,
  square_avg 4.65e-08 / 4.65e-08
* Philox normal, (8200, 3): 1.30e-06 (asserted: 4 times that,
  5.2e-06); (5, 65): 9.70e-07

No kernel exceeded its allowance.
"""
import numpy as np
import pytest
import torch as t

pytestmark = pytest.mark.gpu

if not t.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from machin_amd import ops  # noqa: E402
from machin_amd.ops.sumtree import DeviceSumTree  # noqa: E402
import util_ops_reference as R  # noqa: E402

DEV = "cuda:0"
MARGIN = 8.0
# largest |recovered kernel normal - float64 Box-Muller| over the
# (8200, 3) case of TestGaussianSample, measured on an MI355X; it
# includes the fp32 rounding of the action the noise is recovered from
NOISE_DEV_MEASURED = 1.3e-6
NOISE_TOL = 4.0 * NOISE_DEV_MEASURED
assert NOISE_TOL <= 1e-3

SCAN_IDS = [R.scan_id(s) for s in R.SCAN_SHAPES]


@pytest.fixture(scope="module")
def ext():
    assert ops.available(), "the HIP extension must be built"
    return ops._require_ext()


def gpu(*xs):
    out = tuple(x.to(DEV) for x in xs)
    return out if len(out) > 1 else out[0]


def within(got, want64, bound, what=""):
    err = (got.detach().cpu().double() - want64).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what} worst error {float(err.max()):.3g}, "
          f"worst error/bound {ratio:.3g}")
    return bool((err <= bound).all())


# ======================================================================
# scans
# ======================================================================
class TestScans:
    @pytest.mark.parametrize("gamma", R.SCAN_GAMMAS)
    @pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=SCAN_IDS)
    def test_returns_and_gae(self, shape, gamma):
        c = R.make_scan_case(shape)
        T = shape[0]
        want, M = R.ref_discounted_returns(c["rew"], c["term"], gamma,
                                           c["boot"])
        got = ops.discounted_returns(
            *gpu(c["rew"], c["term"]), gamma, gpu(c["boot"])
        )
        assert got.is_cuda and got.shape == shape
        assert within(got, want, R.scan_bound(R.C_RETURNS, T, M), "returns")
        want, M = R.ref_gae(c["rew"], c["val"], c["next_val"], c["term"],
                            gamma, 0.95)
        got = ops.gae(*gpu(c["rew"], c["val"], c["next_val"], c["term"]),
                      gamma, 0.95)
        assert within(got, want, R.scan_bound(R.C_GAE, T, M), "gae")

    @pytest.mark.parametrize("mode", ["all", "none"])
    def test_bootstrap_with_all_or_no_terminals(self, mode):
        c = R.make_scan_case((7, 65), terminals=mode)
        want, M = R.ref_discounted_returns(c["rew"], c["term"], 0.999,
                                           c["boot"])
        got = ops.discounted_returns(*gpu(c["rew"], c["term"]), 0.999,
                                     gpu(c["boot"]))
        assert within(got, want, R.scan_bound(R.C_RETURNS, 7, M))
        if mode == "all":
            assert t.equal(got.cpu(), c["rew"])
        v = R.make_vtrace_case((7, 65), terminals=mode)
        args = (v["blp"], v["tlp"], v["rew"], v["val"], v["boot"], v["term"])
        vs64, pg64, M = R.ref_vtrace(*args, 0.999, **R.VTRACE_CLIPS_TIGHT)
        vs, pg = ops.vtrace(*gpu(*args), 0.999, **R.VTRACE_CLIPS_TIGHT)
        bound = R.scan_bound(R.C_VTRACE, 7, M)
        assert within(vs, vs64, bound) and within(pg, pg64, bound)

    def test_one_dimensional_form(self):
        c = R.make_scan_case((9, 1), seed=3)
        rew, term = c["rew"][:, 0], c["term"][:, 0]
        want, M = R.ref_discounted_returns(c["rew"], c["term"], 0.999,
                                           c["boot"])
        got = ops.discounted_returns(*gpu(rew, term), 0.999, gpu(c["boot"]))
        assert got.shape == (9,)
        assert within(got.view(9, 1), want,
                      R.scan_bound(R.C_RETURNS, 9, M))
        want, M = R.ref_gae(c["rew"], c["val"], c["next_val"], c["term"],
                            0.999, 0.95)
        got = ops.gae(*gpu(rew, c["val"][:, 0], c["next_val"][:, 0], term),
                      0.999, 0.95)
        assert got.shape == (9,)
        assert within(got.view(9, 1), want, R.scan_bound(R.C_GAE, 9, M))
        want, M = R.ref_nstep_returns(c["rew"], c["term"], 0.999, 3)
        got = ops.nstep_returns(*gpu(rew, term), 0.999, 3)
        assert got.shape == (9,)
        assert within(got.view(9, 1), want, R.scan_bound(R.C_NSTEP, 3, M))

    @pytest.mark.parametrize("shape", R.NSTEP_SHAPES,
                             ids=[R.scan_id(s) for s in R.NSTEP_SHAPES])
    def test_nstep(self, shape):
        c = R.make_scan_case(shape, seed=5)
        T = shape[0]
        rew, term = gpu(c["rew"], c["term"])
        for gamma in R.SCAN_GAMMAS:
            for n in (1, 3, 16, T + 2):
                want, M = R.ref_nstep_returns(c["rew"], c["term"], gamma, n)
                got = ops.nstep_returns(rew, term, gamma, n)
                assert within(
                    got, want, R.scan_bound(R.C_NSTEP, min(n, T), M),
                    f"nstep g={gamma} n={n}",
                ), (gamma, n)

    @pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=SCAN_IDS)
    def test_vtrace_all_clips_active(self, shape):
        c = R.make_vtrace_case(shape, clipped=True)
        args = (c["blp"], c["tlp"], c["rew"], c["val"], c["boot"], c["term"])
        for gamma in R.SCAN_GAMMAS:
            vs64, pg64, M = R.ref_vtrace(*args, gamma,
                                         **R.VTRACE_CLIPS_TIGHT)
            vs, pg = ops.vtrace(*gpu(*args), gamma, **R.VTRACE_CLIPS_TIGHT)
            bound = R.scan_bound(R.C_VTRACE, shape[0], M)
            assert within(vs, vs64, bound, "vs"), gamma
            assert within(pg, pg64, bound, "pg"), gamma

    @pytest.mark.parametrize("shape", [(7, 65), (1000, 3)],
                             ids=["7x65", "1000x3"])
    def test_vtrace_unclipped_measured(self, shape):
        c = R.make_vtrace_case(shape, clipped=False)
        args = (c["blp"], c["tlp"], c["rew"], c["val"], c["boot"], c["term"])
        vs64, pg64, _ = R.ref_vtrace(*args, 0.999, **R.VTRACE_CLIPS_LOOSE)
        cpu = ops.vtrace(*args, 0.999, **R.VTRACE_CLIPS_LOOSE)
        got = ops.vtrace(*gpu(*args), 0.999, **R.VTRACE_CLIPS_LOOSE)
        for name, f, k, w in zip(("vs", "pg_adv"), cpu, got, (vs64, pg64)):
            e_f = float((f.double() - w).abs().max())
            e_k = float((k.cpu().double() - w).abs().max())
            print(f"MEASURED vtrace unclipped {shape} {name}: "
                  f"fallback {e_f:.3g}, kernel {e_k:.3g}")
            assert e_f > 0
            assert e_k <= MARGIN * e_f, name

    @pytest.mark.parametrize("clipped", [True, False],
                             ids=["clipped", "unclipped"])
    @pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=SCAN_IDS)
    def test_vtrace_batch_major_is_bit_equal(self, shape, clipped):
        c = R.make_vtrace_case(shape, clipped=clipped)
        clips = R.VTRACE_CLIPS_TIGHT if clipped else R.VTRACE_CLIPS_LOOSE
        tb = gpu(c["blp"], c["tlp"], c["rew"], c["val"])
        boot, term = gpu(c["boot"], c["term"])
        vs, pg = ops.vtrace(*tb, boot, term, 0.999, **clips)
        vs2, pg2 = ops.vtrace(
            *(x.t().contiguous() for x in tb), boot, term.t().contiguous(),
            0.999, time_major=False, **clips,
        )
        assert vs2.shape == (shape[1], shape[0])
        assert t.equal(vs2.t(), vs) and t.equal(pg2.t(), pg)


# ======================================================================
# categorical projection
# ======================================================================
class TestProjection:
    @staticmethod
    def check(batch, A, v_min, v_max, gamma=0.99):
        dist, rew, term = R.make_projection_case(batch, A, v_min, v_max)
        want = R.ref_projection(dist, rew, term, gamma, v_min, v_max)
        got = ops.categorical_projection(*gpu(dist, rew, term), gamma,
                                         v_min, v_max).cpu().double()
        assert got.shape == (batch, A)
        assert t.allclose(got, want, rtol=R.PROJ_RTOL, atol=R.PROJ_ATOL), \
            (v_min, v_max, A, batch)
        mass = dist.double().sum(dim=1)
        lost = float((got.sum(dim=1) - mass).abs().max())
        assert lost <= R.PROJ_MASS_TOL, (v_min, v_max, A, batch, lost)

    @pytest.mark.parametrize("batch", R.PROJ_BATCHES)
    @pytest.mark.parametrize("v_range", R.PROJ_RANGES,
                             ids=[f"{a:g}_{b:g}" for a, b in R.PROJ_RANGES])
    def test_overshooting_supports(self, v_range, batch):
        atoms = [a for lo, hi, a in R.overshooting_supports()
                 if (lo, hi) == v_range]
        assert atoms
        for A in atoms:
            self.check(batch, A, *v_range)

    @pytest.mark.parametrize("batch", R.PROJ_BATCHES)
    @pytest.mark.parametrize("atoms", [51, 2, 256])
    def test_plain_supports(self, atoms, batch):
        self.check(batch, atoms, -10.0, 10.0)

    @pytest.mark.parametrize("atoms", [51, 124, 256])
    def test_zero_discount(self, atoms):
        self.check(5, atoms, -10.0, 10.0, gamma=0.0)


# ======================================================================
# sum-tree
# ======================================================================
class TestSumTree:
    @pytest.mark.parametrize("size,fill", R.sumtree_cases())
    def test_nodes_and_walk(self, size, fill):
        leaves = R.make_leaf_weights(size, fill)
        tree = DeviceSumTree(size, DEV)
        tree.update_all_leaves(t.from_numpy(leaves))
        cap, depth = tree.capacity, tree.depth
        R.check_tree_nodes(tree.weights.cpu().numpy(), cap, size, leaves)
        for round_no in range(4):
            if round_no:
                w, idx = R.make_update_rounds(size)[round_no - 1]
                tree.update_leaf_batch(t.from_numpy(w), t.from_numpy(idx))
                leaves[idx] = w
                R.check_tree_nodes(tree.weights.cpu().numpy(), cap, size,
                                   leaves)
            if round_no not in (0, 3):
                continue
            nodes = tree.weights.cpu().numpy()
            u = R.sumtree_queries(nodes, cap, size)
            got = tree.find_leaf_index(t.from_numpy(u)).cpu().numpy()
            model = R.sumtree_walk(nodes, u, cap, depth, size)
            assert np.array_equal(got, model), (
                f"{(got != model).sum()} of {u.size} leaves differ from "
                "the walk model"
            )
            R.check_leaves_found(nodes, cap, depth, size, u, got)

    def test_sample_returns_live_leaves(self):
        """``sample`` forms its own queries on the device, u == total
        included for large n."""
        size = 5000
        leaves = R.make_leaf_weights(size, "60%")
        tree = DeviceSumTree(size, DEV)
        tree.update_all_leaves(t.from_numpy(leaves))
        t.manual_seed(0)
        idx = tree.sample(1 << 16).cpu().numpy()
        assert (leaves[idx] > 0).all()


# ======================================================================
# multi-tensor polyak and fused RMSprop
# ======================================================================
class TestPolyak:
    @pytest.mark.parametrize("tau", R.POLYAK_TAUS)
    @pytest.mark.parametrize("name", list(R.MT_LISTS))
    def test_three_entry_points(self, ext, monkeypatch, name, tau):
        tgt, src = R.make_polyak_case(R.MT_LISTS[name])
        want = R.ref_polyak(tgt, src, tau)
        src_d = [x.to(DEV) for x in src]

        def fresh():
            return [x.to(DEV) for x in tgt]

        a = fresh()
        ext.multi_tensor_polyak(a, src_d, tau)
        b = fresh()
        plan = ops.FusedPolyak(b, src_d)
        plan(tau)
        c = fresh()
        monkeypatch.setenv("MACHIN_AMD_FUSED_POLYAK", "1")
        assert ops._use_fused_polyak()
        ops.polyak_update_(c, src_d, tau)
        for i, w in enumerate(want):
            for got in (a[i], b[i], c[i]):
                assert R.ulp_distance_ok(got.cpu(), w), (name, i)
            assert t.equal(a[i], b[i]) and t.equal(a[i], c[i])
        for s, s0 in zip(src_d, src):
            assert t.equal(s.cpu(), s0)

    @pytest.mark.parametrize("tau", R.POLYAK_TAUS)
    def test_mixed_signs(self, ext, tau):
        """Both signs, magnitudes over many binades, zeros: products
        that cancel."""
        tgt, src = R.make_polyak_mixed_case(R.MT_NUMELS)
        got = [x.to(DEV) for x in tgt]
        ext.multi_tensor_polyak(got, [x.to(DEV) for x in src], tau)
        for g, a, b in zip(got, tgt, src):
            assert R.polyak_mixed_ok(g.cpu(), a, b, tau)


class TestFusedRMSprop:
    @pytest.mark.parametrize("name,mode", [
        ("edges", "skip"), ("edges", "clip"), ("edges", "noclip"),
        ("long", "clip"),
    ])
    def test_three_steps_against_float64(self, name, mode):
        max_norm = R.RMS_MAX_NORMS[mode]
        case = R.make_rmsprop_case(R.MT_LISTS[name])
        params, sq, grads = case
        p64, s64 = R.ref_rmsprop(*case, max_norm, **R.RMS_HYPER)
        p32, s32 = R.run_eager_rmsprop(*case, max_norm, **R.RMS_HYPER)
        opt, ps = R.eager_rmsprop(*case, max_norm, device=DEV, **R.RMS_HYPER)
        plan = ops.FusedRMSprop(opt, max_norm=max_norm)
        for step in grads:
            for p, g in zip(ps, step):
                p.grad.copy_(g)
            assert plan.matches(opt)
            plan.step()
        sk = [opt.state[p]["square_avg"] for p in ps]
        for what, ref32, got, w in (("params", p32, ps, p64),
                                    ("square_avg", s32, sk, s64)):
            e_f = R.max_abs_err(ref32, w)
            e_k = R.max_abs_err(got, w)
            print(f"MEASURED rmsprop {name}/{mode} {what}: "
                  f"eager {e_f:.3g}, kernel {e_k:.3g}")
            assert e_f > 0
            assert e_k <= MARGIN * e_f, what
        # gradients are scaled in registers, never written back
        for p, g in zip(ps, grads[-1]):
            assert t.equal(p.grad.cpu(), g)


# ======================================================================
# distributions
# ======================================================================
def flat_index(shape):
    return np.arange(int(np.prod(shape))).reshape(shape)


class TestGaussianSample:
    @pytest.mark.parametrize("shape", R.GAUSS_SHAPES,
                             ids=[R.scan_id(s) for s in R.GAUSS_SHAPES])
    def test_noise_is_philox_and_logp_is_float64(self, ext, shape):
        mu, ls = R.make_gauss_case(shape)
        seed, offset = 1234, 3
        act, logp = ext.gaussian_sample_logprob(*gpu(mu, ls), seed, offset,
                                                False, 1e-6)
        assert act.shape == shape and logp.shape == (shape[0], 1)
        a = act.cpu()
        noise = ((a.double() - mu.double()) * t.exp(-ls.double())).numpy()
        want = R.philox_normal(seed, offset, flat_index(shape))
        dev = np.abs(noise - want).max()
        print(f"MEASURED noise deviation {shape}: {dev:.3g}")
        assert dev <= NOISE_TOL
        want_lp, bound = R.ref_gaussian_logprob(mu, ls, a)
        assert within(logp, want_lp, bound, "logp")

    def test_seed_and_offset_words(self, ext):
        shape = (5, 65)
        mu, ls = gpu(*R.make_gauss_case(shape))
        mu_c, ls_c = mu.cpu().double(), ls.cpu().double()

        def noise(seed, offset):
            act, _ = ext.gaussian_sample_logprob(mu, ls, seed, offset, False,
                                                 1e-6)
            return act, ((act.cpu().double() - mu_c) * t.exp(-ls_c)).numpy()

        big_seed, big_off = (3 << 32) + 17, (5 << 32) + 2
        for seed, offset in ((big_seed, 0), (17, big_off),
                             (big_seed, big_off)):
            _, n = noise(seed, offset)
            want = R.philox_normal(seed, offset, flat_index(shape))
            assert np.abs(n - want).max() <= NOISE_TOL
        a1, _ = noise(big_seed, 7)
        a2, _ = noise(big_seed, 7)
        a3, _ = noise(big_seed, 8)
        a4, _ = noise(17, 7)
        assert t.equal(a1, a2)
        assert not t.equal(a1, a3) and not t.equal(a1, a4)

    def test_squashed_action_is_tanh_of_the_same_sample(self, ext):
        shape = (5, 65)
        mu, ls = R.make_gauss_case(shape)
        act, logp = ext.gaussian_sample_logprob(*gpu(mu, ls), 99, 7, True,
                                                1e-6)
        eps = t.from_numpy(R.philox_normal(99, 7, flat_index(shape)))
        std = t.exp(ls.double())
        u = mu.double() + eps * std
        a64 = t.tanh(u)
        # |d tanh| <= 1: the noise tolerance scaled by std, plus fp32
        tol = NOISE_TOL * std + 4 * R.U24 * (1.0 + u.abs())
        assert bool(((act.cpu().double() - a64).abs() <= tol).all())
        assert float(act.abs().max()) <= 1.0
        term = (-0.5 * eps * eps - ls.double() - R.LOG_SQRT_2PI
                - t.log(1.0 - a64 * a64 + R.f32(1e-6)))
        want = term.sum(dim=1, keepdim=True)
        # d/du log(1 - tanh^2 + e) is at most 2: the sample's tolerance
        # doubled, |eps| times the noise tolerance, the cancellation in
        # the fp32 1 - a^2 + e (a and a^2 rounded, divided by the small
        # sum) and fp32 roundings
        s = 1.0 - a64 * a64 + R.f32(1e-6)
        bound = (2 * tol + eps.abs() * NOISE_TOL
                 + 4 * R.U24 * (a64 * a64 + s) / s
                 + R.C_GAUSS * R.U24 * term.abs()).sum(dim=1, keepdim=True) \
            + 8 * R.U24 * term.abs().sum(dim=1, keepdim=True)
        assert within(logp, want, bound, "squashed logp")


class TestGaussianLogprob:
    @pytest.mark.parametrize("squash", [False, True],
                             ids=["plain", "tanh"])
    @pytest.mark.parametrize("shape", R.GAUSS_SHAPES,
                             ids=[R.scan_id(s) for s in R.GAUSS_SHAPES])
    def test_against_float64(self, ext, shape, squash):
        mu, ls = R.make_gauss_case(shape, seed=1)
        g = t.Generator().manual_seed(11)
        act = t.randn(*shape, generator=g)
        if squash:
            act = t.tanh(act)
            flat = act.view(-1)
            edge = t.tensor([1.0, -1.0, 0.0])[:flat.numel()]
            flat[:edge.numel()] = edge
            flat[-1] = 1.0
        logp = ext.gaussian_logprob(*gpu(mu, ls, act), squash, 1e-6)
        assert logp.shape == (shape[0], 1)
        want, bound = R.ref_gaussian_logprob(mu, ls, act, squash, 1e-6)
        assert bool(t.isfinite(logp).all())
        assert within(logp, want, bound, f"logprob squash={squash}")


class TestNoiseKernels:
    @pytest.mark.parametrize("add", [False, True], ids=["set", "add"])
    @pytest.mark.parametrize("n", [1, R.GRID_THREADS + 3])
    def test_normal_noise(self, ext, n, add):
        g = t.Generator().manual_seed(n)
        x0 = t.randn(n, generator=g)
        x = gpu(x0).clone()
        mean, std, seed, offset = 0.25, 0.5, (1 << 33) + 5, 11
        ext.normal_noise_(x, mean, std, seed, offset, add)
        v = mean + std * R.philox_normal(seed, offset, np.arange(n))
        want = x0.double().numpy() + v if add else v
        err = np.abs(x.cpu().double().numpy() - want)
        tol = std * NOISE_TOL + 3 * R.U24 * (np.abs(want) + np.abs(v) + mean)
        print(f"normal_noise_ n={n} add={add}: worst error {err.max():.3g}")
        assert (err <= tol).all()

    @pytest.mark.parametrize("n", [1, R.GRID_THREADS + 3])
    def test_ou_update(self, ext, n):
        g = t.Generator().manual_seed(n + 1)
        x0 = t.randn(n, generator=g) * 2
        x = gpu(x0).clone()
        mu, theta, sigma, dt, seed, offset = 0.5, 0.15, 0.2, 0.25, 42, 9
        ext.ou_update_(x, mu, theta, sigma, dt, seed, offset)
        x64 = x0.double().numpy()
        noise = R.philox_normal(seed, offset, np.arange(n))
        drift = R.f32(theta) * (R.f32(mu) - x64) * R.f32(dt)
        kick = R.f32(sigma) * float(np.sqrt(np.float32(dt))) * noise
        want = x64 + drift + kick
        err = np.abs(x.cpu().double().numpy() - want)
        tol = R.f32(sigma) * 0.5 * NOISE_TOL + 6 * R.U24 * (
            np.abs(x64) + np.abs(drift) + np.abs(kick) + 1.0
        )
        assert (err <= tol).all()


# ======================================================================
# categorical policy head
# ======================================================================
class TestPolicyHead:
    @pytest.mark.parametrize("rows", R.PG_ROWS)
    @pytest.mark.parametrize("actions", R.PG_ACTIONS)
    def test_forward_and_backward(self, actions, rows):
        logits, act, gt, ge = R.make_pg_case(rows, actions)
        taken64, ent64, grad64 = R.ref_pg_head(logits, act, gt, ge)
        x = gpu(logits).requires_grad_(True)
        taken, ent = ops.categorical_policy_head(x, gpu(act))
        assert taken.dtype == ent.dtype == t.float32
        assert taken.shape == ent.shape == (rows,)
        b_taken, b_ent = R.pg_forward_bounds(actions, taken64, ent64)
        assert within(taken, taken64, b_taken, f"taken A={actions}")
        assert within(ent, ent64, b_ent, f"entropy A={actions}")
        (grad,) = t.autograd.grad([taken, ent], [x], gpu(gt, ge))
        assert grad.dtype == t.bfloat16 and grad.shape == (rows, actions)
        want = grad64.to(t.bfloat16).double()
        err = (grad.cpu().double() - want).abs()
        tol = R.PG_BF16_RTOL * want.abs() + R.PG_BF16_ATOL
        print(f"pg head backward A={actions} N={rows}: worst error/"
              f"tolerance {float((err / tol).max()):.3g}")
        assert bool((err <= tol).all())
        if actions == 1:
            assert not grad.any()  # p == 1: both products vanish


# ======================================================================
# u8 dequantisation
# ======================================================================
class TestDequant:
    @pytest.mark.parametrize("scale", R.DEQUANT_SCALES,
                             ids=["1/255", "1"])
    @pytest.mark.parametrize("n", R.DEQUANT_SIZES)
    def test_exact(self, n, scale):
        g = t.Generator().manual_seed(n)
        x = t.randint(0, 256, (n,), dtype=t.uint8, generator=g)
        if n >= 2:
            x[0], x[-1] = 255, 254
        got = ops.dequant_u8(gpu(x), scale)
        assert got.dtype == t.bfloat16 and got.shape == (n,)
        assert t.equal(got.cpu(), (x.float() * scale).to(t.bfloat16))

    @pytest.mark.parametrize("start", [1, 3])
    @pytest.mark.parametrize("n", [16 * 100 + 5, 16 * R.GRID_THREADS + 9])
    def test_unaligned_slices(self, n, start):
        """A contiguous slice whose storage offset is no multiple of
        16 takes the scalar kernel for the whole range."""
        g = t.Generator().manual_seed(n + start)
        x = t.randint(0, 256, (n,), dtype=t.uint8, generator=g)
        xd = gpu(x)
        assert xd.data_ptr() % 16 == 0
        part = xd[start:]
        assert part.is_contiguous() and part.data_ptr() % 16 == start
        got = ops.dequant_u8(part, 1.0 / 255.0)
        want = (x[start:].float() * (1.0 / 255.0)).to(t.bfloat16)
        assert t.equal(got.cpu(), want)


# ======================================================================
# argument checks of the bindings (all raise before any launch)
# ======================================================================
class TestBindingChecks:
    def test_scans(self, ext):
        f = lambda *s: t.zeros(*s, device=DEV)  # noqa: E731
        T, B = 4, 6
        with pytest.raises(RuntimeError):
            ext.discounted_returns(f(T, B), f(T, B - 1), f(B), 0.9)
        with pytest.raises(RuntimeError):
            ext.discounted_returns(f(T, B), f(T, B), f(B - 1), 0.9)
        with pytest.raises(RuntimeError):
            ext.discounted_returns(f(T, B), f(T, B), f(B).double(), 0.9)
        with pytest.raises(RuntimeError):
            ext.discounted_returns(f(T, B), f(T, B), t.zeros(B), 0.9)
        with pytest.raises(RuntimeError):
            ext.discounted_returns(f(T * B), f(T * B), f(B), 0.9)
        with pytest.raises(RuntimeError):
            ext.gae(f(T, B), f(T - 1, B), f(T, B), f(T, B), 0.9, 0.9)
        with pytest.raises(RuntimeError):
            ext.gae(f(T, B), f(T, B), f(T, B).double(), f(T, B), 0.9, 0.9)
        with pytest.raises(RuntimeError):
            ext.gae(f(T, B), f(T, B), f(T, B), f(T, B)[:, :3], 0.9, 0.9)
        with pytest.raises(RuntimeError):
            ext.nstep_returns(f(T, B), f(T, B - 1), 0.9, 3)
        for fn in (ext.vtrace, ext.vtrace_bt):
            ok = [f(T, B) for _ in range(4)] + [f(B), f(T, B)]
            if fn is ext.vtrace_bt:
                ok = [f(B, T) for _ in range(4)] + [f(B), f(B, T)]
            fn(*ok, 0.9, 1.0, 1.0, 1.0)
            for i in (0, 1, 3, 4, 5):
                bad = list(ok)
                bad[i] = f(bad[i].numel() - 1)
                with pytest.raises(RuntimeError):
                    fn(*bad, 0.9, 1.0, 1.0, 1.0)
            bad = list(ok)
            bad[4] = bad[4].half()
            with pytest.raises(RuntimeError):
                fn(*bad, 0.9, 1.0, 1.0, 1.0)

    def test_projection_and_gaussians(self, ext):
        f = lambda *s: t.zeros(*s, device=DEV)  # noqa: E731
        B, A = 5, 51
        with pytest.raises(RuntimeError):
            ext.categorical_projection(f(B, A), f(B - 1), f(B), 0.9, -1., 1.)
        with pytest.raises(RuntimeError):
            ext.categorical_projection(f(B, A), f(B), f(B).double(), 0.9,
                                       -1., 1.)
        with pytest.raises(RuntimeError):
            ext.categorical_projection(f(B, 1), f(B), f(B), 0.9, -1., 1.)
        with pytest.raises(RuntimeError):
            ext.categorical_projection(f(B, 257), f(B), f(B), 0.9, -1., 1.)
        D = 3
        with pytest.raises(RuntimeError):
            ext.gaussian_sample_logprob(f(B, D), f(B, D - 1), 1, 0, False,
                                        1e-6)
        with pytest.raises(RuntimeError):
            ext.gaussian_sample_logprob(f(B, D), f(B, D).double(), 1, 0,
                                        False, 1e-6)
        with pytest.raises(RuntimeError):
            ext.gaussian_logprob(f(B, D), f(B, D), f(B - 1, D), False, 1e-6)
        with pytest.raises(RuntimeError):
            ext.gaussian_logprob(f(B, D), f(B, 1), f(B, D), False, 1e-6)
        with pytest.raises(RuntimeError):
            ext.gaussian_logprob(f(B, D), f(B, D), f(B, D).double(), True,
                                 1e-6)

    def test_policy_head(self, ext):
        N, A = 7, 6
        logits = t.zeros(N, A, device=DEV, dtype=t.bfloat16)
        act = t.zeros(N, device=DEV, dtype=t.int64)
        g = t.zeros(N, device=DEV)
        ext.pg_head_fwd(logits, act)
        ext.pg_head_bwd(logits, act, g, g)
        wide = t.zeros(N, 33, device=DEV, dtype=t.bfloat16)
        with pytest.raises(RuntimeError):
            ext.pg_head_fwd(wide, act)
        with pytest.raises(RuntimeError):
            ext.pg_head_bwd(wide, act, g, g)
        with pytest.raises(RuntimeError):
            ext.pg_head_fwd(logits, act[:-1])
        with pytest.raises(RuntimeError):
            ext.pg_head_fwd(logits, act.int())
        with pytest.raises(RuntimeError):
            ext.pg_head_fwd(logits, act.cpu())
        with pytest.raises(RuntimeError):
            ext.pg_head_bwd(logits, act[:-1], g, g)
        with pytest.raises(RuntimeError):
            ext.pg_head_bwd(logits, act, g[:-1], g)
        with pytest.raises(RuntimeError):
            ext.pg_head_bwd(logits, act, g, g.double())
        with pytest.raises(RuntimeError):
            ext.pg_head_bwd(logits.float(), act, g, g)

    def test_sumtree(self, ext):
        cap, depth = 8, 3
        tree = t.zeros(2 * cap, device=DEV)
        idx = t.zeros(4, device=DEV, dtype=t.int64)
        w = t.ones(4, device=DEV)
        u = t.zeros(4, device=DEV)
        ext.sumtree_update(tree, idx, w, cap, depth)
        ext.sumtree_build(tree, cap)
        ext.sumtree_sample(tree, u, cap, depth, cap)
        with pytest.raises(RuntimeError):
            ext.sumtree_update(tree, idx, w[:-1], cap, depth)
        with pytest.raises(RuntimeError):
            ext.sumtree_update(tree, idx.int(), w, cap, depth)
        with pytest.raises(RuntimeError):
            ext.sumtree_update(tree, idx, w.double(), cap, depth)
        with pytest.raises(RuntimeError):
            ext.sumtree_update(tree[:-2], idx, w, cap, depth)
        with pytest.raises(RuntimeError):
            ext.sumtree_update(tree, idx, w, cap, depth + 1)
        with pytest.raises(RuntimeError):
            ext.sumtree_build(tree[:-2], cap)
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(tree, u.double(), cap, depth, cap)
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(tree[:-2], u, cap, depth, cap)
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(tree, u, cap, depth, cap + 1)
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(tree, u.cpu(), cap, depth, cap)
        # a tree that starts off an 8-byte boundary (the walk loads
        # child pairs)
        odd = t.zeros(2 * cap + 1, device=DEV)[1:]
        assert odd.data_ptr() % 8 == 4
        with pytest.raises(RuntimeError):
            ext.sumtree_sample(odd, u, cap, depth, cap)
