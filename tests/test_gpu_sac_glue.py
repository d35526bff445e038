"""GPU tests of the SAC learn step's native glue kernels: critic loss, actor
loss, the sampler on the raw actor head, twin Adam + polyak, and the replay
gather. The torch composition that the agent ran before these kernels (and
still runs under ``rl.sac.FORCE_TORCH_GLUE``) is the oracle throughout, and
every fused expression rounds where the separate torch kernels round, so the
comparisons are bit for bit (torch.equal) except for the loss values, which
feed nothing but backward() and are summed in another order (1e-6 relative).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import smartcal_amd.ops as ops
    DEV = torch.device("cuda:0")
else:
    DEV = None

BATCHES = [1, 3, 8, 64, 65]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_hip(), "HIP extension must be loaded on a GPU box"


@pytest.fixture
def torch_glue():
    """Context switch: `with torch_glue(True):` forces the torch
    composition of the glue; always restored."""
    from smartcal_amd.rl import sac

    class _Force:
        def __init__(self, on):
            self.on = on

        def __enter__(self):
            sac.FORCE_TORCH_GLUE = self.on

        def __exit__(self, *exc):
            sac.FORCE_TORCH_GLUE = False

    yield _Force
    sac.FORCE_TORCH_GLUE = False


def _col(B, g, scale=1.0):
    return (torch.randn(B, 1, generator=g) * scale).to(DEV)


# ---- 1. critic loss -------------------------------------------------------

def _critic_inputs(B):
    g = torch.Generator().manual_seed(100 + B)
    q1, q2, q1_t, q2_t = (_col(B, g) for _ in range(4))
    logp = _col(B, g, 3.0)
    reward = _col(B, g, 20.0)
    rows = torch.arange(B, device=DEV).unsqueeze(1)
    q2_t = torch.where(rows % 4 == 2, q1_t, q2_t)     # ties in the target
    done = rows % 3 == 0                              # some terminal rows
    return q1, q2, q1_t, q2_t, logp, reward, done


def _critic_composition(q1, q2, q1_t, q2_t, logp, reward, done, alpha,
                        gamma):
    with torch.no_grad():
        t = torch.min(q1_t, q2_t) - alpha * logp
        t = t.masked_fill(done, 0.0)
        y = reward + gamma * t
    return F.mse_loss(q1, y) + F.mse_loss(q2, y), y


@pytest.mark.parametrize("alpha", [0.03, 0.0])
@pytest.mark.parametrize("B", BATCHES)
def test_critic_loss_matches_composition(B, alpha):
    from smartcal_amd.rl.sac import sac_critic_loss
    q1, q2, q1_t, q2_t, logp, reward, done = _critic_inputs(B)
    alpha_t = torch.tensor(alpha, device=DEV)
    gamma = 0.99
    a1, a2 = q1.clone().requires_grad_(), q2.clone().requires_grad_()
    b1, b2 = q1.clone().requires_grad_(), q2.clone().requires_grad_()
    loss_ref, y_ref = _critic_composition(a1, a2, q1_t, q2_t, logp, reward,
                                          done, alpha_t, gamma)
    loss_ref.backward()
    loss, y = sac_critic_loss(b1, b2, q1_t, q2_t, logp, reward, done,
                              alpha_t, gamma)
    assert not y.requires_grad
    loss.backward()
    loss, loss_ref = loss.detach(), loss_ref.detach()
    print(f"B={B} alpha={alpha}: loss {float(loss)!r} ref "
          f"{float(loss_ref)!r}; dq1 mismatches "
          f"{int((b1.grad != a1.grad).sum())}, dq2 "
          f"{int((b2.grad != a2.grad).sum())}, y "
          f"{int((y != y_ref).sum())}")
    assert torch.equal(y, y_ref)
    assert torch.equal(b1.grad, a1.grad)
    assert torch.equal(b2.grad, a2.grad)
    assert float(a1.grad.abs().max()) > 0
    assert abs(float(loss) - float(loss_ref)) <= 1e-6 * abs(float(loss_ref))


def test_critic_loss_passes_target_nan():
    from smartcal_amd.rl.sac import sac_critic_loss
    q1, q2, q1_t, q2_t, logp, reward, done = _critic_inputs(8)
    assert not bool(done[1])
    q1_t[1] = float("nan")
    _, y = sac_critic_loss(q1, q2, q1_t, q2_t, logp, reward, done,
                           torch.tensor(0.03, device=DEV), 0.99)
    nan = torch.isnan(y).view(-1)
    assert bool(nan[1]) and int(nan.sum()) == 1


# ---- 2. actor loss --------------------------------------------------------

def _actor_inputs(B):
    g = torch.Generator().manual_seed(200 + B)
    q1, q2 = _col(B, g), _col(B, g)
    logp = _col(B, g, 3.0)
    rows = torch.arange(B, device=DEV).unsqueeze(1)
    q2 = torch.where(rows % 3 == 0, q1, q2)           # ties
    q2 = torch.where(rows % 3 == 1, q1 + 0.5, q2)     # q1 < q2
    q2 = torch.where(rows % 3 == 2, q1 - 0.5, q2)     # q1 > q2
    return q1, q2, logp


def _actor_grads(fn, q1, q2, logp):
    leaves = [t.clone().requires_grad_() for t in (q1, q2, logp)]
    loss = fn(*leaves)
    loss.backward()
    return loss.detach(), [t.grad for t in leaves]


@pytest.mark.parametrize("B", BATCHES)
def test_actor_loss_matches_composition(B):
    from smartcal_amd.rl.sac import sac_actor_loss
    q1, q2, logp = _actor_inputs(B)
    alpha = torch.tensor(0.03, device=DEV)
    loss_ref, ref = _actor_grads(
        lambda a, b, lp: (alpha * lp - torch.min(a, b)).mean(), q1, q2, logp)
    loss, got = _actor_grads(
        lambda a, b, lp: sac_actor_loss(a, b, lp, alpha), q1, q2, logp)
    for name, a, b in zip(("dq1", "dq2", "dlogp"), got, ref):
        print(f"B={B} {name}: mismatches {int((a != b).sum())}")
        assert torch.equal(a, b), name
    assert float(ref[2].abs().max()) > 0
    assert abs(float(loss) - float(loss_ref)) \
        <= 1e-6 * max(abs(float(loss_ref)), 1e-3)


def test_actor_loss_nan_row_feeds_both_critics():
    """torch.minimum's derivative sends the whole gradient to both operands
    of a row where neither comparison holds."""
    from smartcal_amd.rl.sac import sac_actor_loss
    q1, q2, logp = _actor_inputs(8)
    q1[5] = float("nan")
    alpha = torch.tensor(0.03, device=DEV)
    _, ref = _actor_grads(
        lambda a, b, lp: (alpha * lp - torch.min(a, b)).mean(), q1, q2, logp)
    _, got = _actor_grads(
        lambda a, b, lp: sac_actor_loss(a, b, lp, alpha), q1, q2, logp)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert float(got[0][5]) == float(got[1][5]) == -0.125


# ---- 3. sampler on the raw actor head -------------------------------------

# raw logsigma values: below, on and above both clamp bounds, and inside
_RAW = [-25.0, -20.0, -3.25, 0.5, 2.0, 7.0]


@pytest.mark.parametrize("A", [1, 2, 65])
@pytest.mark.parametrize("B", [1, 3, 17])
def test_head_sample_matches_slice_clamp_sample(B, A):
    from smartcal_amd.ops.sampling import (tanh_gauss_head_sample,
                                           tanh_gauss_sample)
    from smartcal_amd.rl.networks import LOGSIG_MAX, LOGSIG_MIN
    g = torch.Generator().manual_seed(10 * B + A)
    n = B * A
    # a shape with fewer logsigma values than _RAW runs once per start
    for start in range(1 if n >= len(_RAW) else len(_RAW)):
        raw = torch.tensor([_RAW[(start + i) % len(_RAW)] for i in range(n)])
        out = torch.cat((torch.randn(B, A, generator=g), raw.view(B, A)),
                        dim=1).to(DEV)
        eps = torch.randn(B, A, generator=g).to(DEV)
        w_a = torch.randn(B, A, generator=g).to(DEV)
        w_l = torch.randn(B, 1, generator=g).to(DEV)

        o_ref = out.clone().requires_grad_()
        a_ref, lp_ref = tanh_gauss_sample(
            o_ref[:, :A], o_ref[:, A:].clamp(LOGSIG_MIN, LOGSIG_MAX), 1.0,
            True, eps=eps)
        ((a_ref * w_a).sum() + (lp_ref * w_l).sum()).backward()

        o_new = out.clone().requires_grad_()
        a_new, lp_new = tanh_gauss_head_sample(o_new, LOGSIG_MIN, LOGSIG_MAX,
                                               1.0, True, eps=eps)
        ((a_new * w_a).sum() + (lp_new * w_l).sum()).backward()

        assert a_new.shape == (B, A) and lp_new.shape == (B, 1)
        assert torch.equal(a_new, a_ref)
        assert torch.equal(lp_new, lp_ref)
        assert torch.equal(o_new.grad, o_ref.grad)
        assert torch.isfinite(o_new.grad).all()
        # outside the bounds the logsigma gradient is cut, on them it is not
        cut = (raw < LOGSIG_MIN) | (raw > LOGSIG_MAX)
        dls = o_new.grad[:, A:].reshape(-1).cpu()
        assert bool((dls[cut] == 0).all())
        assert bool((dls[~cut] != 0).all())

        with torch.no_grad():
            a_ng, lp_ng = tanh_gauss_head_sample(out, LOGSIG_MIN, LOGSIG_MAX,
                                                 1.0, False, eps=eps)
        assert torch.equal(a_ng, a_ref) and torch.equal(lp_ng, lp_ref)


@pytest.mark.parametrize("B", [1, 8])
def test_sample_normal_draws_the_same_noise(B, torch_glue):
    from smartcal_amd.rl.networks import SACActorMLP
    torch.manual_seed(3)
    actor = SACActorMLP(24, 2).to(DEV)
    state = torch.randn(B, 24, device=DEV)
    res = []
    for forced in (True, False):
        with torch_glue(forced):
            torch.manual_seed(11)
            a, lp = actor.sample_normal(state, reparameterize=True)
            (a.sum() + lp.sum()).backward()
            grads = [p.grad.clone() for p in actor.parameters()]
            actor.zero_grad(set_to_none=True)
            with torch.no_grad():
                a2, lp2 = actor.sample_normal(state[0], reparameterize=False)
            nxt = torch.randn(5, device=DEV)     # the generator moved alike
        res.append((a.detach(), lp.detach(), a2, lp2, nxt, *grads))
    for x, y in zip(*res):
        assert x.shape == y.shape
        assert torch.equal(x, y)


# ---- 4. twin Adam + polyak ------------------------------------------------

class _Pool(torch.nn.Module):
    def __init__(self, values):
        super().__init__()
        self.w = torch.nn.Parameter(values.clone())


@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_adam_polyak_pair_matches_separate_launches(n):
    from smartcal_amd.utils.flatten import FlatParams, FusedAdam
    g = torch.Generator().manual_seed(n)
    init = [torch.randn(n, generator=g).to(DEV) for _ in range(4)]
    grads = [[(torch.randn(n, generator=g) * 0.1).to(DEV) for _ in range(2)]
             for _ in range(3)]

    def build():
        fps = [FlatParams(_Pool(v).to(DEV)) for v in init]
        opts = [FusedAdam(fps[0], lr=1e-3), FusedAdam(fps[1], lr=1e-3)]
        return fps, opts

    fps_r, opts_r = build()
    fps_n, opts_n = build()
    for step, tau in enumerate((0.005, 0.4, 0.6)):
        for k in range(2):
            fps_r[k].flat_grad.copy_(grads[step][k])
            fps_n[k].flat_grad.copy_(grads[step][k])
        opts_r[0].step()
        opts_r[1].step()
        fps_r[2].polyak_from(fps_r[0], tau)
        fps_r[3].polyak_from(fps_r[1], tau)
        FusedAdam.step_pair_polyak(opts_n[0], opts_n[1], fps_n[2], fps_n[3],
                                   tau)
        for k in range(4):
            bad = int((fps_n[k].flat != fps_r[k].flat).sum())
            print(f"n={n} step {step} tau {tau} pool {k}: mismatches {bad}")
            assert torch.equal(fps_n[k].flat, fps_r[k].flat), (step, k)
        for a, b in zip(opts_n, opts_r):
            assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
            assert torch.equal(a.t_dev, b.t_dev)
            assert a.step_count == b.step_count == step + 1
            assert float(a.state_dict()["t_dev"]) == step + 1
    assert not torch.equal(fps_n[2].flat, init[2])


# ---- 5. replay gather -----------------------------------------------------

@pytest.mark.parametrize("D", [1, 24, 420])
def test_replay_gather_matches_index_select(D):
    rows, B, A, scale = 5, 3, 2, 20
    g = torch.Generator().manual_seed(D)
    state = torch.randn(rows, D, generator=g).to(DEV)
    new_state = torch.randn(rows, D, generator=g).to(DEV)
    action = torch.randn(rows, A, generator=g).to(DEV)
    reward = torch.randn(rows, generator=g).to(DEV)
    terminal = torch.tensor([False, True, False, False, True], device=DEV)
    idx = torch.tensor([4, 1, 4], device=DEV)

    def outs():
        return (torch.zeros(B, D, device=DEV), torch.zeros(B, D, device=DEV),
                torch.zeros(B, A, device=DEV), torch.zeros(B, 1, device=DEV),
                torch.zeros(B, 1, dtype=torch.bool, device=DEV))

    ref = outs()
    torch.index_select(state, 0, idx, out=ref[0])
    torch.index_select(new_state, 0, idx, out=ref[1])
    torch.index_select(action, 0, idx, out=ref[2])
    torch.index_select(reward, 0, idx, out=ref[3].view(-1))
    ref[3].mul_(scale)
    torch.index_select(terminal, 0, idx, out=ref[4].view(-1))

    got = outs()
    ops.ext().replay_gather(idx, state, new_state, action, reward, terminal,
                            float(scale), *got)
    for a, b in zip(got, ref):
        assert torch.equal(a, b)
    assert bool(got[4].any()) and float(got[0].abs().max()) > 0

    with pytest.raises(RuntimeError):
        ops.ext().replay_gather(idx.int(), state, new_state, action, reward,
                                terminal, float(scale), *outs())
    with pytest.raises(RuntimeError):
        ops.ext().replay_gather(idx[:2], state, new_state, action, reward,
                                terminal, float(scale), *outs())


# ---- 6. a SAC agent, native glue against the torch glue -------------------

def _sac_pools(forced, graphed, torch_glue):
    from smartcal_amd.rl.sac import Agent
    np.random.seed(0)
    torch.manual_seed(0)
    with torch_glue(forced):
        agent = Agent(gamma=0.99, batch_size=8, n_actions=2, tau=0.005,
                      max_mem_size=64, input_dims=[24], lr_a=1e-3,
                      lr_c=1e-3, reward_scale=2, alpha=0.03, device=DEV)
        rng = np.random.default_rng(1)
        obs = {"eig": torch.from_numpy(rng.standard_normal(8)).float(),
               "A": torch.from_numpy(rng.standard_normal(16)).float()}
        for i in range(10):
            a = agent.choose_action(obs)
            obs2 = {"eig": torch.from_numpy(rng.standard_normal(8)).float(),
                    "A": torch.from_numpy(rng.standard_normal(16)).float()}
            agent.store_transition(obs, a, 0.25 * (i % 3), obs2, i == 4,
                                   np.zeros(2, np.float32))
            obs = obs2
        if graphed:
            agent.enable_cuda_graph()
        for _ in range(3):
            agent.learn()
        torch.cuda.synchronize()
    assert agent.learn_counter == 3
    assert agent.critic_1_opt.step_count == agent.critic_2_opt.step_count
    assert float(agent.critic_1_opt.t_dev) == float(agent.actor_opt.t_dev)
    return [fp.flat.clone() for fp in (
        agent.actor_fp, agent.critic_1_fp, agent.critic_2_fp,
        agent.target_critic_1_fp, agent.target_critic_2_fp)]


@pytest.mark.parametrize("graphed", [False, True])
def test_sac_learn_matches_torch_glue(graphed, torch_glue):
    """Three learn steps from one seed: the five flat parameter pools with
    the native glue (eager, and captured into a hipGraph) equal those of the
    torch composition run the same way."""
    native = _sac_pools(False, graphed, torch_glue)
    comp = _sac_pools(True, graphed, torch_glue)
    for i, (a, b) in enumerate(zip(native, comp)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"pool {i}"
