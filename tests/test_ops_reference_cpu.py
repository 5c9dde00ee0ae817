"""The float64 references and host models of ``util_ops_reference``
against the fp32 CPU fallbacks of ``machin_amd.ops``, before either
judges a HIP kernel (``test_ops_edges_gpu.py``). Runs anywhere.

* Philox4x32-10 passes the published known-answer vectors.
* Scans: fallback within the derived bound ``c T 2^-24 M`` of the
  float64 recurrence (the unclipped V-trace case gets 4 more roundings
  per step for the fp32 exponential and ratio).
* Projection: the ``(range, atoms)`` combinations whose fp32 position
  overshoots the support are enumerated, not hard-coded; on each the
  fallback matches the float64 reference and conserves mass.
* Sum-tree: the numpy walk model equals the CPU ``DeviceSumTree`` path
  and returns no zero-weight leaf for any query in ``[0, total]``; the
  same model without the zero-subtree guard does, which is what the
  checks are there to catch.
"""
import numpy as np
import pytest
import torch as t

from machin_amd import ops
from machin_amd.ops.sumtree import DeviceSumTree
import util_ops_reference as R

SCAN_IDS = [R.scan_id(s) for s in R.SCAN_SHAPES]


def within(got, want64, bound):
    """|got - want| <= bound elementwise; reports the worst ratio."""
    err = (got.double() - want64).abs()
    ok = bool((err <= bound).all())
    if not ok:
        ratio = (err / bound.clamp_min(1e-300)).max()
        print(f"worst error/bound = {float(ratio):.3g}, "
              f"worst error = {float(err.max()):.3g}")
    return ok


class TestPhilox:
    def test_known_answer_vectors(self):
        for ctr, key, want in R.PHILOX_KAT:
            got = R.philox4x32_10(ctr, key)
            assert tuple(int(x[0]) for x in got) == want

    def test_vectorised_equals_scalar(self):
        idx = np.arange(5, dtype=np.uint64)
        many = R.philox4x32_10((7, 0, idx, 0), (3, 9))
        for i in range(5):
            one = R.philox4x32_10((7, 0, i, 0), (3, 9))
            assert [int(x[i]) for x in many] == [int(x[0]) for x in one]

    def test_uniform_map_is_the_kernels(self):
        u = R.philox_uniform(np.array([0, 0xFF, 0x100, 0xFFFFFFFF]))
        assert u[0] == 2.0 ** -25 and u[1] == 2.0 ** -25
        assert u[2] == float(np.float32(2.0 ** -24 + 2.0 ** -25))
        # (1 - 2^-24) + 2^-25 is a tie in fp32 and rounds to 1.0
        assert u[3] == 1.0
        assert (u > 0).all() and (u <= 1).all()

    def test_normal_moments_and_layout(self):
        n = R.philox_normal(1234, 0, np.arange(200000))
        assert abs(n.mean()) < 0.01 and abs(n.std() - 1.0) < 0.01
        # seed and offset above 2^32 reach the high words
        a = R.philox_normal(5, 0, np.arange(8))
        assert not np.array_equal(a, R.philox_normal(5 + (1 << 32), 0,
                                                     np.arange(8)))
        assert not np.array_equal(a, R.philox_normal(5, 1 << 32,
                                                     np.arange(8)))
        assert not np.array_equal(a, R.philox_normal(5, 1, np.arange(8)))
        assert R.philox_normal(5, 0, np.arange(6).reshape(2, 3)).shape \
            == (2, 3)


class TestScanFallbacks:
    @pytest.mark.parametrize("gamma", R.SCAN_GAMMAS)
    @pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=SCAN_IDS)
    def test_returns_and_gae(self, shape, gamma):
        c = R.make_scan_case(shape)
        T = shape[0]
        want, M = R.ref_discounted_returns(c["rew"], c["term"], gamma,
                                           c["boot"])
        got = ops.discounted_returns(c["rew"], c["term"], gamma, c["boot"])
        assert within(got, want, R.scan_bound(R.C_RETURNS, T, M))
        want, M = R.ref_gae(c["rew"], c["val"], c["next_val"], c["term"],
                            gamma, 0.95)
        got = ops.gae(c["rew"], c["val"], c["next_val"], c["term"], gamma,
                      0.95)
        assert within(got, want, R.scan_bound(R.C_GAE, T, M))

    @pytest.mark.parametrize("mode", ["all", "none"])
    def test_bootstrap_with_all_or_no_terminals(self, mode):
        c = R.make_scan_case((7, 65), terminals=mode)
        want, M = R.ref_discounted_returns(c["rew"], c["term"], 0.999,
                                           c["boot"])
        if mode == "all":
            # the bootstrap never enters
            assert t.equal(want, c["rew"].double())
        got = ops.discounted_returns(c["rew"], c["term"], 0.999, c["boot"])
        assert within(got, want, R.scan_bound(R.C_RETURNS, 7, M))

    def test_one_dimensional_form(self):
        c = R.make_scan_case((9, 1), seed=3)
        want, M = R.ref_discounted_returns(c["rew"], c["term"], 0.999,
                                           c["boot"])
        got = ops.discounted_returns(c["rew"][:, 0], c["term"][:, 0], 0.999,
                                     c["boot"])
        assert got.shape == (9,)
        assert within(got.view(9, 1), want, R.scan_bound(R.C_RETURNS, 9, M))

    @pytest.mark.parametrize("shape", R.NSTEP_SHAPES,
                             ids=[R.scan_id(s) for s in R.NSTEP_SHAPES])
    def test_nstep(self, shape):
        c = R.make_scan_case(shape, seed=5)
        T = shape[0]
        for gamma in R.SCAN_GAMMAS:
            for n in (1, 3, 16, T + 2):
                want, M = R.ref_nstep_returns(c["rew"], c["term"], gamma, n)
                got = ops.nstep_returns(c["rew"], c["term"], gamma, n)
                assert within(
                    got, want, R.scan_bound(R.C_NSTEP, min(n, T), M)
                ), (gamma, n)

    def test_nstep_reference_is_the_definition(self):
        """The vectorised reference against the plain double loop."""
        c = R.make_scan_case((6, 2), seed=9)
        rew, term = c["rew"].double(), c["term"].double()
        for n in (1, 3, 8):
            want = t.zeros(6, 2, dtype=t.float64)
            for i in range(6):
                for b in range(2):
                    alive, disc = 1.0, 1.0
                    for k in range(n):
                        if i + k >= 6:
                            break
                        want[i, b] += disc * alive * rew[i + k, b]
                        alive *= 1.0 - float(term[i + k, b])
                        disc *= R.f32(0.999)
            got, _ = R.ref_nstep_returns(c["rew"], c["term"], 0.999, n)
            assert t.allclose(got, want, rtol=1e-13, atol=1e-13)

    @pytest.mark.parametrize("clipped", [True, False],
                             ids=["clipped", "unclipped"])
    @pytest.mark.parametrize("shape", R.SCAN_SHAPES, ids=SCAN_IDS)
    def test_vtrace(self, shape, clipped):
        c = R.make_vtrace_case(shape, clipped=clipped)
        clips = R.VTRACE_CLIPS_TIGHT if clipped else R.VTRACE_CLIPS_LOOSE
        args = (c["blp"], c["tlp"], c["rew"], c["val"], c["boot"], c["term"])
        vs64, pg64, M = R.ref_vtrace(*args, 0.999, **clips)
        vs, pg = ops.vtrace(*args, 0.999, **clips)
        # unclipped: the fp32 difference, exponential and ratio product
        k = R.C_VTRACE + (0 if clipped else 4)
        bound = R.scan_bound(k, shape[0], M)
        assert within(vs, vs64, bound)
        assert within(pg, pg64, bound)

    def test_vtrace_batch_major_fallback(self):
        c = R.make_vtrace_case((7, 65), clipped=False)
        args = (c["blp"], c["tlp"], c["rew"], c["val"])
        vs, pg = ops.vtrace(*args, c["boot"], c["term"], 0.999)
        vs2, pg2 = ops.vtrace(
            *(x.t().contiguous() for x in args), c["boot"],
            c["term"].t().contiguous(), 0.999, time_major=False,
        )
        assert t.equal(vs2, vs.t()) and t.equal(pg2, pg.t())


class TestProjectionFallback:
    def test_overshooting_supports_exist(self):
        over = R.overshooting_supports()
        assert over, "no support overshoots: the cases select nothing"
        assert (-10.0, 10.0, 124) in over and (0.0, 1.0, 62) in over
        assert (-10.0, 10.0, 51) not in over

    @pytest.mark.parametrize("v_range", R.PROJ_RANGES,
                             ids=[f"{a:g}_{b:g}" for a, b in R.PROJ_RANGES])
    def test_matches_float64_and_conserves_mass(self, v_range):
        v_min, v_max = v_range
        atoms = [a for lo, hi, a in R.overshooting_supports()
                 if (lo, hi) == v_range]
        if v_range == (-10.0, 10.0):
            atoms += [51, 2, 256]
        assert atoms
        for A in atoms:
            for batch in (1, 5):
                dist, rew, term = R.make_projection_case(batch, A, v_min,
                                                         v_max)
                want = R.ref_projection(dist, rew, term, 0.99, v_min, v_max)
                got = ops.categorical_projection(dist, rew, term, 0.99,
                                                 v_min, v_max)
                assert t.allclose(got.double(), want, rtol=R.PROJ_RTOL,
                                  atol=R.PROJ_ATOL), (A, batch)
                mass = dist.double().sum(dim=1)
                assert float((got.double().sum(dim=1) - mass).abs().max()) \
                    <= R.PROJ_MASS_TOL, (A, batch)
                assert float((want.sum(dim=1) - mass).abs().max()) < 1e-12

    def test_reward_far_above_the_support_on_the_last_row(self):
        """The reported failure: IndexError from bin ``A`` of the last
        row with a reward of ``3 v_max`` on (-10, 10, 124)."""
        dist = t.full((2, 124), 1.0 / 124)
        rew = t.tensor([0.0, 30.0])
        got = ops.categorical_projection(dist, rew, t.zeros(2), 0.99,
                                         -10.0, 10.0)
        assert float(got[1, 123]) == pytest.approx(1.0, abs=1e-5)
        assert float(got[1, :123].abs().max()) <= 1e-5


class TestGaussianReference:
    @pytest.mark.parametrize("squash", [False, True])
    def test_against_torch_distributions(self, squash):
        mu, ls = R.make_gauss_case((5, 65))
        g = t.Generator().manual_seed(1)
        act = t.randn(5, 65, generator=g)
        if squash:
            act = t.tanh(act)
            act[0, :3] = t.tensor([1.0, -1.0, 0.0])
        got, bound = R.ref_gaussian_logprob(mu, ls, act, squash, 1e-6)
        a = act.double()
        corr = 0.0
        if squash:
            lim = float(np.float32(1.0) - np.float32(1e-6))
            c = a.clamp(-lim, lim)
            corr = t.log(1.0 - c * c + R.f32(1e-6))
            a = t.atanh(c)
        d = t.distributions.Normal(mu.double(), ls.double().exp())
        want = (d.log_prob(a) - corr).sum(dim=1, keepdim=True)
        assert t.allclose(got, want, rtol=1e-12, atol=1e-10)
        # an fp32 evaluation of the same formula stays inside the bound
        d32 = t.distributions.Normal(mu, ls.exp())
        a32 = act
        corr32 = 0.0
        if squash:
            c32 = act.clamp(-1 + 1e-6, 1 - 1e-6)
            corr32 = t.log(1.0 - c32 * c32 + 1e-6)
            a32 = 0.5 * (t.log(1 + c32) - t.log(1 - c32))
        fp32 = (d32.log_prob(a32) - corr32).sum(dim=1, keepdim=True)
        assert within(fp32, got, bound)
        assert float(bound.max()) < (0.2 if squash else 1e-3)


class TestSumTreeModel:
    @pytest.mark.parametrize("size,fill", R.sumtree_cases())
    def test_walk_model_and_invariants(self, size, fill):
        leaves = R.make_leaf_weights(size, fill)
        tree = DeviceSumTree(size, "cpu")
        tree.update_all_leaves(t.from_numpy(leaves))
        cap, depth = tree.capacity, tree.depth
        R.check_tree_nodes(tree.weights.numpy(), cap, size, leaves)
        for round_no in range(4):
            if round_no:
                w, idx = R.make_update_rounds(size)[round_no - 1]
                tree.update_leaf_batch(t.from_numpy(w), t.from_numpy(idx))
                leaves[idx] = w
                R.check_tree_nodes(tree.weights.numpy(), cap, size, leaves)
            if round_no not in (0, 3):
                continue
            nodes = tree.weights.numpy()
            u = R.sumtree_queries(nodes, cap, size)
            model = R.sumtree_walk(nodes, u, cap, depth, size)
            # the model alone: no zero-weight leaf on [0, total]
            R.check_leaves_found(nodes, cap, depth, size, u, model)
            got = tree.find_leaf_index(t.from_numpy(u)).numpy()
            assert np.array_equal(got, model)

    def test_unguarded_walk_returns_dead_leaves(self):
        """What the guard is for: the walk that never looks at the
        right child fails the same check (u == 0 enters the dead first
        leaf, u == total can run into padding)."""
        failed = 0
        for size, fill in R.sumtree_cases():
            if size == 1:
                continue
            leaves = R.make_leaf_weights(size, fill)
            tree = DeviceSumTree(size, "cpu")
            tree.update_all_leaves(t.from_numpy(leaves))
            nodes = tree.weights.numpy()
            u = R.sumtree_queries(nodes, tree.capacity, size)
            bad = R.sumtree_walk(nodes, u, tree.capacity, tree.depth, size,
                                 rule=R.rule_unguarded)
            try:
                R.check_leaves_found(nodes, tree.capacity, tree.depth, size,
                                     u, bad)
            except AssertionError:
                failed += 1
        assert failed == len(R.sumtree_cases()) - 2  # all but size 1

    def test_stratified_sample_can_reach_the_total(self):
        """``rand + (n - 1)`` rounds to ``n`` in fp32 for large n, so
        ``sample`` itself forms u == total."""
        n = np.float32(1 << 20)
        top = np.float32(1.0 - 2.0 ** -24) + (n - np.float32(1.0))
        assert top == n


class TestMultiTensorReferences:
    @pytest.mark.parametrize("tau", R.POLYAK_TAUS)
    @pytest.mark.parametrize("name", ["edges", "many"])
    def test_polyak_fallback(self, name, tau):
        tgt, src = R.make_polyak_case(R.MT_LISTS[name])
        want = R.ref_polyak(tgt, src, tau)
        ops.polyak_update_(tgt, src, tau)
        for got, w in zip(tgt, want):
            assert R.ulp_distance_ok(got, w)

    @pytest.mark.parametrize("tau", R.POLYAK_TAUS)
    def test_polyak_fallback_mixed_signs(self, tau):
        tgt, src = R.make_polyak_mixed_case(R.MT_NUMELS)
        tgt0 = [x.clone() for x in tgt]
        ops.polyak_update_(tgt, src, tau)
        for got, a, b in zip(tgt, tgt0, src):
            assert R.polyak_mixed_ok(got, a, b, tau)

    @pytest.mark.parametrize("mode", list(R.RMS_MAX_NORMS))
    def test_rmsprop_reference_against_eager(self, mode):
        max_norm = R.RMS_MAX_NORMS[mode]
        params, sq, grads = R.make_rmsprop_case(R.MT_NUMELS)
        p64, s64 = R.ref_rmsprop(params, sq, grads, max_norm, **R.RMS_HYPER)
        ps, ss = R.run_eager_rmsprop(params, sq, grads, max_norm,
                                     **R.RMS_HYPER)
        err_p = R.max_abs_err(ps, p64)
        err_s = R.max_abs_err(ss, s64)
        print(f"eager fp32 vs float64 ({mode}): params {err_p:.3g}, "
              f"square_avg {err_s:.3g}")
        # fp32 parameters of magnitude <= 8 round at 2^-22 per step
        assert 0 < err_p < 3 * 3 * 2.0 ** -22
        assert 0 < err_s < 1e-4
        # the three modes differ: clipping changed the result
        if mode == "clip":
            raw, _ = R.ref_rmsprop(params, sq, grads, 0.0, **R.RMS_HYPER)
            assert R.max_abs_err([x.float() for x in raw], p64) > 1e-3


class TestPolicyHeadReference:
    @pytest.mark.parametrize("actions", R.PG_ACTIONS)
    def test_forward_and_gradient(self, actions):
        logits, act, gt, ge = R.make_pg_case(300, actions)
        taken64, ent64, grad64 = R.ref_pg_head(logits, act, gt, ge)
        taken, ent = ops.categorical_policy_head(logits, act)
        b_taken, b_ent = R.pg_forward_bounds(actions, taken64, ent64)
        assert within(taken, taken64, b_taken)
        assert within(ent, ent64, b_ent)
        # the analytic gradient against float64 autograd
        x = logits.double().requires_grad_(True)
        logp = t.log_softmax(x, dim=-1)
        tl = logp.gather(1, act.view(-1, 1)).view(-1)
        en = -(logp.exp() * logp).sum(dim=-1)
        ((tl * gt.double()).sum() + (en * ge.double()).sum()).backward()
        assert t.allclose(x.grad, grad64, rtol=1e-10, atol=1e-12)


class TestDequantFallback:
    @pytest.mark.parametrize("scale", R.DEQUANT_SCALES)
    def test_every_byte_value(self, scale):
        x = t.arange(256, dtype=t.uint8)
        want = (x.float() * scale).to(t.bfloat16)
        assert t.equal(ops.dequant_u8(x, scale), want)
