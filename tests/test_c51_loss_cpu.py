"""``ops.c51_loss`` on the CPU fallback path and the RAINBOW options
built on it (``fused_loss``, ``dist_from_logits``,
``exact_nstep_bootstrap``).

Tolerances: the fallback against the eager chain of ``RAINBOW.update``
is the same fp32 arithmetic (``atol=1e-6``); against the float64
reference ``rtol=1e-4, atol=1e-3``, the project's projection tolerance,
in the older tests. That ``atol`` is the size of a typical element of
``proj``, so ``TestHatReference`` holds the fallback (``loss``, ``proj``
and the gradient) to the per-element worst-case rounding bound derived
in ``util_c51_loss.reference_hat``, on every edge case and support of
``util_c51_loss.EDGE_CASES``, and checks the bound itself: a typical
bound is below 1/1000 of a typical element, and six deliberately wrong
references differ from the true one by more than twice the bound.
"""
import numpy as np
import pytest
import torch as t

from machin_amd import ops
from machin_amd.frame.algorithms import RAINBOW
from machin_amd.frame.buffers import DeviceFrameStackBuffer
from util_c51_loss import (
    ATOL, EDGE_CASES, RTOL, SMALL_SHAPES, V_MAX, V_MIN, WRONG_CASES,
    WRONG_VARIANTS, FixedLogitsNet, LogitsQNet, PixelDistQNet,
    build_rainbow, edge_id, edge_reference, expected_logits_loss,
    fallback_edge_result, make_case, make_edge_case, make_tie_case, op_args,
    pixel_episode, record_update, reference64, reference_hat, seed_all,
    seeded_update, shape_id, taken_rows, worst_ratio,
)

SHAPE_IDS = [shape_id(s) for s in SMALL_SHAPES]


def eager_chain(dist, action, next_online, next_target, reward, terminal,
                gamma_n, v_min, v_max):
    """The loss chain of ``RAINBOW.update`` without ``fused_loss``,
    from the three distributions to ``per_sample``."""
    B, A, N = dist.shape
    device = dist.device
    with t.no_grad():
        support = t.linspace(v_min, v_max, N, device=device)
        next_q = (next_online * support.view(1, 1, N)).sum(dim=2)
        best = next_q.argmax(dim=1)
        next_dist = next_target[t.arange(B, device=device), best]
        reward = reward.to(device).float().view(B)
        terminal = terminal.to(device).float().view(B)
        proj = ops.categorical_projection(
            next_dist, reward, terminal, gamma_n, v_min, v_max
        )
    pred = dist[t.arange(B, device=device), action]
    log_pred = t.log(pred.clamp_min(1e-8))
    return -(proj * log_pred).sum(dim=1), proj, best


class TestFallback:
    @pytest.mark.parametrize("shape", SMALL_SHAPES, ids=SHAPE_IDS)
    def test_equals_eager_chain(self, shape):
        case = make_case(shape, t.float32, False)
        gamma_n = 0.99 ** 3
        args = op_args(case, discount=gamma_n)
        loss, proj, best = ops._c51_loss_torch(*args, from_logits=False)
        want_loss, want_proj, want_best = eager_chain(*args)
        assert t.equal(best, want_best)
        assert t.allclose(proj, want_proj, rtol=0, atol=1e-6)
        assert t.allclose(loss, want_loss, rtol=0, atol=1e-6)

    @pytest.mark.parametrize("from_logits", [False, True],
                             ids=["prob", "logits"])
    @pytest.mark.parametrize("shape", SMALL_SHAPES, ids=SHAPE_IDS)
    def test_against_float64(self, shape, from_logits):
        case = make_case(shape, t.float32, from_logits)
        loss, proj, best = ops.c51_loss(
            *op_args(case), from_logits=from_logits
        )
        want_loss, want_proj, want_best = reference64(case)
        assert loss.dtype == proj.dtype == t.float32
        assert best.dtype == t.int64
        assert loss.shape == best.shape == (shape[0],)
        assert proj.shape == (shape[0], shape[2])
        assert t.equal(best, want_best) and t.equal(best, case.best)
        assert t.allclose(proj.double(), want_proj, rtol=RTOL, atol=ATOL)
        assert t.allclose(loss.double(), want_loss, rtol=RTOL, atol=ATOL)

    def test_bf16_inputs_compute_in_fp32(self):
        case = make_case((5, 3, 51), t.bfloat16, True)
        got = ops.c51_loss(*op_args(case), from_logits=True)
        want = ops.c51_loss(*op_args(case, upcast=True), from_logits=True)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and t.equal(g, w)

    def test_gradcheck_logits(self):
        case = make_case((5, 3, 51), t.float32, True)
        args = list(op_args(case))
        for i in (0, 2, 3):
            args[i] = args[i].double()
        args[0].requires_grad_(True)

        def fn(dist):
            return ops._c51_loss_torch(dist, *args[1:], from_logits=True)[0]

        assert t.autograd.gradcheck(fn, (args[0],))

    def test_only_loss_is_differentiable(self):
        case = make_case((5, 3, 51), t.float32, True)
        args = list(op_args(case))
        args[0] = args[0].clone().requires_grad_(True)
        loss, proj, best = ops.c51_loss(*args, from_logits=True)
        assert loss.requires_grad
        assert not proj.requires_grad and not best.requires_grad
        loss.sum().backward()
        taken = t.zeros(5, 3, dtype=t.bool)
        taken[t.arange(5), case.action] = True
        assert bool((args[0].grad[~taken] == 0).all())
        assert bool((args[0].grad[taken] != 0).any())

    def test_rejects_bad_arguments(self):
        case = make_case((5, 3, 51), t.float32, True)
        names = ("dist", "action", "next_online", "next_target", "reward",
                 "terminal", "discount", "v_min", "v_max")
        good = dict(zip(names, op_args(case)))
        ops.c51_loss(**good)

        def wide(a, n):
            return {k: t.zeros(5, a, n) for k in
                    ("dist", "next_online", "next_target")}

        for bad in (
            dict(next_online=good["next_online"].bfloat16()),  # dtype mix
            dict(next_target=good["next_target"].double()),
            wide(3, 1), wide(3, 257), wide(65, 51),
            dict(next_online=good["next_online"][:4]),
            dict(dist=good["dist"][0]),
            dict(action=good["action"][:4]),
            dict(action=good["action"].int()),
            dict(reward=good["reward"][:4]),
            dict(terminal=good["terminal"][:4]),
            dict(discount=good["discount"][:4]),
            dict(discount=good["discount"].double()),
            dict(v_min=10.0, v_max=-10.0),
        ):
            with pytest.raises(ValueError):
                ops.c51_loss(**{**good, **bad})

    def test_accepts_column_shapes(self):
        case = make_case((5, 3, 51), t.float32, True)
        args = list(op_args(case))
        want = ops.c51_loss(*args, from_logits=True)
        for i in (1, 4, 5):
            args[i] = args[i].view(-1, 1)
        args[5] = args[5] > 0.5  # terminal as bool
        got = ops.c51_loss(*args, from_logits=True)
        for g, w in zip(got, want):
            assert t.equal(g, w)

    def test_out_of_range_action_is_clamped(self):
        case = make_case((5, 3, 51), t.float32, True)
        args = list(op_args(case))
        wild = t.tensor([-3, 3 + 5, 1, -(2 ** 40), 2 ** 40])
        args[1] = wild
        got = ops.c51_loss(*args, from_logits=True)
        args[1] = wild.clamp(0, 2)
        want = ops.c51_loss(*args, from_logits=True)
        for g, w in zip(got, want):
            assert t.equal(g, w)

    def test_exported(self):
        assert "c51_loss" in ops.__all__


# -- the hat-form reference and its bound ----------------------------------
MODES = pytest.mark.parametrize("from_logits", [False, True],
                                ids=["prob", "logits"])
EDGE = pytest.mark.parametrize("case_key", EDGE_CASES,
                               ids=[edge_id(c) for c in EDGE_CASES])
OUTPUTS = ("loss", "proj", "grad")


class TestHatReference:
    @MODES
    @EDGE
    def test_agrees_with_reference64(self, case_key, from_logits):
        case = make_edge_case(*case_key, t.float32, from_logits)
        ref, _ = edge_reference(case_key, t.float32, from_logits)
        want_loss, want_proj, want_best = reference64(case)
        assert t.equal(ref.best, want_best) and t.equal(ref.best, case.best)
        # float64 rounding: the two forms order the sums differently
        assert float((ref.proj - want_proj).abs().max()) <= 1e-12
        assert t.allclose(ref.loss, want_loss, rtol=1e-12, atol=1e-12)

    @MODES
    @pytest.mark.parametrize("shape", [(5, 3, 51), (9, 4, 124)],
                             ids=shape_id)
    def test_gradient_is_the_float64_autograd(self, shape, from_logits):
        case = make_edge_case(shape, V_MIN, V_MAX, t.float32, from_logits)
        ref, _ = edge_reference((shape, V_MIN, V_MAX), t.float32,
                                from_logits)
        args = list(op_args(case))
        for i in (0, 2, 3):
            args[i] = args[i].double()
        args[0].requires_grad_(True)
        loss, _, _ = ops._c51_loss_torch(*args, from_logits=from_logits)
        (grad,) = t.autograd.grad(loss, args[0], case.g.double())
        rows, others_zero = taken_rows(grad, case)
        assert others_zero
        assert t.allclose(rows, ref.grad, rtol=1e-10, atol=1e-12)

    @MODES
    @EDGE
    def test_fallback_is_within_the_bound(self, case_key, from_logits):
        """A condition on the bound: a second fp32 evaluation, in
        another order than the kernel's, must fit under it."""
        case = make_edge_case(*case_key, t.float32, from_logits)
        ref, bound = edge_reference(case_key, t.float32, from_logits)
        loss, proj, best, grad = fallback_edge_result(case)
        rows, others_zero = taken_rows(grad, case)
        assert others_zero
        assert t.equal(best, ref.best)
        for name, got in zip(OUTPUTS, (loss, proj, rows)):
            ratio, ok = worst_ratio(got, getattr(ref, name),
                                    getattr(bound, name))
            print(f"{name} worst error/bound {ratio:.3g}")
            assert ok, name

    def test_bound_is_tight(self):
        """The tightening over ``atol=1e-3``: on the (67, 18, 65)
        logits case the median bound of ``proj`` is at most 1/1000 of
        the median element of ``proj``, which itself is only a few
        times ``atol``."""
        ref, bound = reference_hat(make_case((67, 18, 65), t.float32, True))
        median = float(ref.proj.median())
        assert 0.0 < median < 10 * ATOL
        assert float(bound.proj.median()) <= median / 1000
        # the edge case of that shape has more empty bins than filled
        # ones; among the filled ones the same holds
        ref, bound = edge_reference(((67, 18, 65), V_MIN, V_MAX),
                                    t.float32, True)
        filled = ref.proj > 0
        assert float(bound.proj[filled].median()) \
            <= float(ref.proj[filled].median()) / 1000

    @MODES
    @pytest.mark.parametrize("case_key", WRONG_CASES,
                             ids=[edge_id(c) for c in WRONG_CASES])
    def test_wrong_references_exceed_the_bound(self, case_key, from_logits):
        """Each wrong variant of the reference differs from the true one
        by more than twice the bound somewhere, so a result within the
        bound of the truth (the fallback above, the kernel on the
        device) cannot be within the bound of a variant. Dropping ``S``
        from the logits gradient is left out: ``S = sum(proj)`` is 1
        here, so that is not observable."""
        case = make_edge_case(*case_key, t.float32, from_logits)
        ref, bound = edge_reference(case_key, t.float32, from_logits)
        for variant in WRONG_VARIANTS:
            wrong, _ = reference_hat(case, wrong=variant)
            seen = False
            for name in OUTPUTS:
                gap = (getattr(wrong, name) - getattr(ref, name)).abs()
                seen |= bool((gap > 2 * getattr(bound, name)).any())
            assert seen, variant

    @MODES
    def test_tie_goes_to_the_lower_action(self, from_logits):
        case = make_tie_case(t.float32, from_logits)
        _, _, best = ops.c51_loss(*op_args(case), from_logits=from_logits)
        assert t.equal(best, case.best)
        assert t.equal(reference_hat(case)[0].best, case.best)


# -- RAINBOW ---------------------------------------------------------------
class TestRainbowFusedLoss:
    def test_same_step_as_eager(self):
        eager, fused = build_rainbow(), build_rainbow(fused_loss=True)
        assert not eager.fused_loss and fused.fused_loss
        before = [p.detach().clone() for p in fused.qnet.parameters()]
        loss_eager, loss_fused = seeded_update(eager), seeded_update(fused)
        assert np.isfinite(loss_eager)
        assert abs(loss_eager - loss_fused) <= 1e-6
        for p, q, p0 in zip(eager.qnet.parameters(),
                            fused.qnet.parameters(), before):
            assert not t.equal(q, p0)
            assert t.allclose(p, q, rtol=0, atol=1e-6)
        for p, q in zip(eager.qnet_target.parameters(),
                        fused.qnet_target.parameters()):
            assert t.allclose(p, q, rtol=0, atol=1e-6)

    def test_options_need_fused_loss(self):
        for option in ("dist_from_logits", "exact_nstep_bootstrap"):
            with pytest.raises(ValueError, match="fused_loss"):
                build_rainbow(**{option: True})

    def test_exact_bootstrap_needs_step_counts(self):
        algo = build_rainbow(fused_loss=True, exact_nstep_bootstrap=True)
        with pytest.raises(ValueError, match="DeviceFrameStackBuffer"):
            algo.update()

    def test_config_forwards_options(self):
        config = RAINBOW.generate_config({})
        fc = config["frame_config"]
        fc["models"] = ["machin_amd.auto.model_zoo.DistQNet"] * 2
        fc["fused_loss"] = True
        algo = RAINBOW.init_from_config(config)
        assert algo.fused_loss and not algo.dist_from_logits
        assert not algo.exact_nstep_bootstrap

    def test_logits_model_acts_on_softmaxed_values(self):
        """Logits whose greedy action differs with and without the
        softmax: acting must apply it."""
        seed_all(0)
        algo = RAINBOW(
            FixedLogitsNet(), FixedLogitsNet(), t.optim.Adam, V_MIN, V_MAX,
            fused_loss=True, dist_from_logits=True,
        )
        state = {"state": t.rand(5, 4)}
        logits = algo.qnet(state["state"])
        z = t.linspace(V_MIN, V_MAX, 3)
        raw = (logits * z).sum(dim=-1).argmax(dim=1)
        want = (t.softmax(logits, dim=-1) * z).sum(dim=-1).argmax(dim=1)
        assert want.tolist() == [0] * 5 and raw.tolist() == [1] * 5
        assert t.equal(algo.act_discrete(state), want.view(-1, 1))
        algo.epsilon = 0.0  # greedy branch
        assert t.equal(algo.act_discrete_with_noise(state),
                       want.view(-1, 1))
        q = algo._q_values(logits)
        assert t.allclose(q[0], t.tensor([8.6413, 5.0]), atol=1e-3)

    def test_logits_model_update(self, monkeypatch):
        """The update passes the logits on as logits and returns the
        IS-weighted mean of -sum(proj * log_softmax), recomputed here
        in float64 from the tensors that reached the op."""
        algo = build_rainbow(net=LogitsQNet, fused_loss=True,
                             dist_from_logits=True)
        calls = record_update(monkeypatch, algo)
        before = [p.detach().clone() for p in algo.qnet.parameters()]
        loss = seeded_update(algo)
        (call,) = calls
        assert call.kwargs["from_logits"] is True
        # the model's raw outputs reached the op: rows do not sum to 1
        row_sums = call.args[0].detach().sum(dim=-1)
        assert float((row_sums - 1.0).abs().min()) > 1e-3
        want = expected_logits_loss(call)
        assert np.isfinite(loss)
        assert loss == pytest.approx(want, rel=RTOL, abs=ATOL)
        assert all(not t.equal(p, p0)
                   for p, p0 in zip(algo.qnet.parameters(), before))

    def test_probability_model_update_is_not_from_logits(self, monkeypatch):
        algo = build_rainbow(fused_loss=True)
        calls = record_update(monkeypatch, algo)
        seeded_update(algo)
        (call,) = calls
        assert call.kwargs["from_logits"] is False
        row_sums = call.args[0].detach().sum(dim=-1)
        assert float((row_sums - 1.0).abs().max()) < 1e-5


class TestExactNStepBootstrap:
    def test_discount_is_gamma_to_the_steps(self, monkeypatch):
        buf = DeviceFrameStackBuffer(
            60, "cpu", n_step=3, discount=0.9, prioritized=True
        )
        algo = RAINBOW(
            PixelDistQNet(), PixelDistQNet(), t.optim.Adam, V_MIN, V_MAX,
            batch_size=16, reward_future_steps=3, discount=0.9,
            replay_buffer=buf, fused_loss=True, exact_nstep_bootstrap=True,
        )
        algo.store_episode(pixel_episode(5))
        sampled, passed = [], []
        real_sample, real_loss = buf.sample_batch, ops.c51_loss

        def sample_batch(*args, **kwargs):
            out = real_sample(*args, **kwargs)
            sampled.append(out[1][-1]["n_step"].view(-1).clone())
            return out

        def c51_loss(*args, **kwargs):
            passed.append(args[6])
            return real_loss(*args, **kwargs)

        monkeypatch.setattr(buf, "sample_batch", sample_batch)
        monkeypatch.setattr(ops, "c51_loss", c51_loss)
        seed_all(3)  # sampling is deterministic from here
        losses = [algo.update() for _ in range(4)]
        assert all(np.isfinite(v) for v in losses)
        assert len(sampled) == len(passed) == 4
        seen = set()
        for steps, discount in zip(sampled, passed):
            assert t.is_tensor(discount) and discount.dtype == t.float32
            assert discount.shape == (16,)
            want = t.tensor(0.9, dtype=t.float64) ** steps.double()
            assert t.allclose(discount.double(), want, rtol=1e-6, atol=0)
            seen |= set(steps.tolist())
        # 0.9, 0.81 and 0.729 all occurred
        assert seen == {1, 2, 3}

    def test_scalar_discount_without_the_option(self, monkeypatch):
        buf = DeviceFrameStackBuffer(
            60, "cpu", n_step=3, discount=0.9, prioritized=True
        )
        algo = RAINBOW(
            PixelDistQNet(), PixelDistQNet(), t.optim.Adam, V_MIN, V_MAX,
            batch_size=16, reward_future_steps=3, discount=0.9,
            replay_buffer=buf, fused_loss=True,
        )
        algo.store_episode(pixel_episode(5))
        passed = []
        real_loss = ops.c51_loss

        def c51_loss(*args, **kwargs):
            passed.append(args[6])
            return real_loss(*args, **kwargs)

        monkeypatch.setattr(ops, "c51_loss", c51_loss)
        assert np.isfinite(algo.update())
        assert passed == [0.9 ** 3]
