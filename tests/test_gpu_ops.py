"""GPU numerics tests: every HIP kernel against its plain-PyTorch fp32
oracle (the CPU implementations in smartcal_amd.ops)."""

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


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_hip(), "HIP extension must be loaded on a GPU box"


def test_fused_linear_fwd_matches_cpu():
    for (B, K, N) in [(64, 420, 512), (1, 420, 512), (64, 512, 256),
                      (64, 128, 4), (3, 33, 17), (64, 320, 1),
                      (4, 7, 64), (20, 7, 64), (5, 2, 192),
                      (4, 64, 192)]:
        x = torch.randn(B, K)
        W = torch.randn(N, K) * 0.05
        b = torch.randn(N) * 0.1
        g = torch.rand(N) + 0.5
        be = torch.randn(N) * 0.1
        ref = F.elu(F.layer_norm(F.linear(x, W, b), (N,), g, be))
        y, zhat, rstd = ops.ext().fused_linear_fwd(
            x.to(DEV), W.to(DEV), b.to(DEV), g.to(DEV), be.to(DEV), 1, True)
        assert torch.allclose(y.cpu(), ref, atol=2e-4), \
            f"shape {(B, K, N)} max err {(y.cpu()-ref).abs().max()}"
        # no-LN + no-act path
        ref2 = F.linear(x, W, b)
        y2, _, _ = ops.ext().fused_linear_fwd(
            x.to(DEV), W.to(DEV), b.to(DEV), None, None, 0, False)
        assert torch.allclose(y2.cpu(), ref2, atol=2e-4)


# dgamma/dbeta column sums take two paths in the backward kernel: loads
# issued early when B <= 64 and each workgroup owns <= 8 columns
# ((64, 420, 512); (40, 9, 200) leaves some waves one or no column), else
# a loop ((4, 7, 64), (5, 2, 192); (100, 9, 64) has more rows than a wave
# and more workgroups than columns).
@pytest.mark.parametrize("B,K,N", [(64, 420, 512), (4, 7, 64),
                                   (5, 2, 192), (40, 9, 200),
                                   (100, 9, 64)])
def test_fused_linear_backward_matches_cpu(B, K, N):
    torch.manual_seed(0)
    x = torch.randn(B, K)
    W = torch.randn(N, K) * 0.05
    b = torch.randn(N) * 0.1
    g = torch.rand(N) + 0.5
    be = torch.randn(N) * 0.1

    # CPU oracle grads
    xc = x.clone().requires_grad_(True)
    Wc = W.clone().requires_grad_(True)
    bc = b.clone().requires_grad_(True)
    gc = g.clone().requires_grad_(True)
    bec = be.clone().requires_grad_(True)
    out = F.elu(F.layer_norm(F.linear(xc, Wc, bc), (N,), gc, bec))
    loss = (out * torch.arange(N).float() / N).sum()
    loss.backward()

    from smartcal_amd.ops.linear import fused_linear
    xg = x.clone().to(DEV).requires_grad_(True)
    Wg = W.clone().to(DEV).requires_grad_(True)
    bg = b.clone().to(DEV).requires_grad_(True)
    gg = g.clone().to(DEV).requires_grad_(True)
    beg = be.clone().to(DEV).requires_grad_(True)
    outg = fused_linear(xg, Wg, bg, gg, beg, act="elu")
    assert torch.allclose(outg.detach().cpu(), out.detach(), atol=2e-4)
    lossg = (outg * (torch.arange(N, device=DEV).float() / N)).sum()
    lossg.backward()

    for cpu_t, gpu_t, name, tol in [
            (xc.grad, xg.grad, "dx", 5e-4),
            (Wc.grad, Wg.grad, "dW", 5e-4),
            (bc.grad, bg.grad, "db", 5e-4),
            (gc.grad, gg.grad, "dgamma", 5e-4),
            (bec.grad, beg.grad, "dbeta", 5e-4)]:
        err = (gpu_t.cpu() - cpu_t).abs().max()
        denom = cpu_t.abs().max().clamp_min(1.0)
        assert err / denom < tol, f"{name}: rel err {err/denom}"


@pytest.mark.parametrize("B,N", [(64, 512), (100, 192)])
def test_fused_linear_backward_bitwise_reproducible(B, N):
    """Same inputs -> the same gradient bits on every run (the column
    sums have a fixed order; no float atomics)."""
    from smartcal_amd.ops.linear import fused_linear
    torch.manual_seed(0)
    K = 33
    x = torch.randn(B, K, device=DEV)
    params = [torch.randn(N, K, device=DEV) * 0.05,
              torch.randn(N, device=DEV) * 0.1,
              torch.rand(N, device=DEV) + 0.5,
              torch.randn(N, device=DEV) * 0.1]
    w = torch.randn(B, N, device=DEV)
    runs = []
    for _ in range(4):
        xs = x.clone().requires_grad_(True)
        ps = [p.clone().requires_grad_(True) for p in params]
        (fused_linear(xs, *ps, act="elu") * w).sum().backward()
        runs.append([t.grad.clone() for t in [xs] + ps])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


def _fused_linear_case(B, N, K=33):
    torch.manual_seed(0)
    x = torch.randn(B, K, device=DEV)
    params = [torch.randn(N, K, device=DEV) * 0.05,
              torch.randn(N, device=DEV) * 0.1,
              torch.rand(N, device=DEV) + 0.5,
              torch.randn(N, device=DEV) * 0.1]
    w = torch.randn(B, N, device=DEV)
    return x, params, w


@pytest.mark.parametrize("B,N", [(64, 512), (100, 192)])
def test_fused_linear_backward_adds_to_existing_grad(B, N):
    """The backward adds into .grad: a second backward without zeroing
    leaves every parameter gradient at twice the first (both column-sum
    paths; x + x is exact in fp32, so the comparison is too)."""
    from smartcal_amd.ops.linear import fused_linear
    x, params, w = _fused_linear_case(B, N)
    ps = [p.clone().requires_grad_(True) for p in params]
    (fused_linear(x, *ps, act="elu") * w).sum().backward()
    once = [p.grad.clone() for p in ps]
    assert all(float(g.abs().max()) > 0 for g in once)
    (fused_linear(x, *ps, act="elu") * w).sum().backward()
    for g1, p, name in zip(once, ps, ["dW", "db", "dgamma", "dbeta"]):
        assert torch.equal(p.grad, g1 + g1), name


@pytest.mark.parametrize("B,N", [(64, 512), (100, 192)])
def test_fused_linear_backward_frozen_params(B, N):
    """Frozen parameters (the actor phase's critics): dgamma/dbeta sums
    are skipped, dx is the same as with live parameters and no parameter
    gets a gradient."""
    from smartcal_amd.ops.linear import fused_linear
    x, params, w = _fused_linear_case(B, N)
    xl = x.clone().requires_grad_(True)
    live = [p.clone().requires_grad_(True) for p in params]
    (fused_linear(xl, *live, act="elu") * w).sum().backward()
    xf = x.clone().requires_grad_(True)
    frozen = [p.clone() for p in params]
    (fused_linear(xf, *frozen, act="elu") * w).sum().backward()
    assert torch.equal(xf.grad, xl.grad)
    assert all(p.grad is None for p in frozen)


def test_mfma_gemms_match_torch():
    A = torch.randn(64, 512)
    B = torch.randn(512, 420)
    C = ops.ext().mfma_gemm_nn(A.to(DEV), B.to(DEV))
    ref = A @ B
    assert torch.allclose(C.cpu(), ref, atol=ref.abs().max() * 1e-5 + 1e-4)

    dz = torch.randn(64, 512)
    x = torch.randn(64, 420)
    dW, db = ops.ext().mfma_gemm_tn_bias(dz.to(DEV), x.to(DEV))
    refW = dz.t() @ x
    assert torch.allclose(dW.cpu(), refW,
                          atol=refW.abs().max() * 1e-5 + 1e-4)
    assert torch.allclose(db.cpu(), dz.sum(0), atol=1e-3)


def test_tanh_gauss_matches_cpu():
    from smartcal_amd.ops.sampling import tanh_gauss_sample
    B, A = 64, 2
    mu = torch.randn(B, A)
    ls = torch.randn(B, A) * 0.3
    eps = torch.randn(B, A)

    a_cpu, lp_cpu = tanh_gauss_sample(
        mu.clone().requires_grad_(True), ls.clone().requires_grad_(True),
        1.0, True, eps)
    mug = mu.clone().to(DEV).requires_grad_(True)
    lsg = ls.clone().to(DEV).requires_grad_(True)
    a_gpu, lp_gpu = tanh_gauss_sample(mug, lsg, 1.0, True, eps.to(DEV))
    assert torch.allclose(a_gpu.detach().cpu(), a_cpu.detach(), atol=1e-5)
    assert torch.allclose(lp_gpu.detach().cpu(), lp_cpu.detach(), atol=1e-4)

    (a_gpu.sum() + lp_gpu.sum()).backward()
    muc = mu.clone().requires_grad_(True)
    lsc = ls.clone().requires_grad_(True)
    a2, lp2 = tanh_gauss_sample(muc, lsc, 1.0, True, eps)
    (a2.sum() + lp2.sum()).backward()
    assert torch.allclose(mug.grad.cpu(), muc.grad, atol=1e-3)
    assert torch.allclose(lsg.grad.cpu(), lsc.grad, atol=1e-3)


def test_fused_adam_matches_torch_adam():
    n = 10_000
    p0 = torch.randn(n)
    g = torch.randn(n)
    # torch reference
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=1e-3)
    p_ref.grad = g.clone()
    for _ in range(3):
        opt.step()
    # fused
    p = p0.clone().to(DEV)
    m = torch.zeros(n, device=DEV)
    v = torch.zeros(n, device=DEV)
    t_dev = torch.zeros(1, device=DEV)
    for _ in range(3):
        ops.ext().fused_adam(p, g.to(DEV), m, v, t_dev, 1e-3, 0.9, 0.999,
                             1e-8)
    assert float(t_dev) == 3.0
    assert torch.allclose(p.cpu(), p_ref.detach(), atol=1e-5)


def test_enet_solver_matches_reference():
    from smartcal_amd.ops import enet as enet_ops
    torch.manual_seed(3)
    N = M = 20
    for trial in range(3):
        A = torch.randn(N, M)
        A /= A.norm()
        y = torch.randn(N) * 0.3
        rho1, rho2 = 0.05, 0.01
        x_ref, opt = enet_ops.lbfgs_solve_reference(A, y, rho1, rho2)

        Ab = A.unsqueeze(0).to(DEV).contiguous()
        yb = y.unsqueeze(0).to(DEV).contiguous()
        rho = torch.tensor([[rho1, rho2]], device=DEV)
        xg, Yg, Sg, nh = ops.ext().enet_lbfgs_solve(Ab, yb, rho, 20, 10, 7)
        torch.cuda.synchronize()

        def loss_of(xv):
            e = y - A @ xv
            return float(e.dot(e) + rho1 * xv.dot(xv)
                         + rho2 * xv.abs().sum())

        l_ref = loss_of(x_ref)
        l_gpu = loss_of(xg[0].cpu())
        assert abs(l_gpu - l_ref) <= 0.02 * abs(l_ref) + 1e-5, \
            f"trial {trial}: gpu loss {l_gpu} vs ref {l_ref}"
        assert int(nh[0]) > 0


def test_enet_influence_matches_reference():
    from smartcal_amd.ops import enet as enet_ops
    torch.manual_seed(4)
    N = M = 20
    A = torch.randn(N, M)
    A /= A.norm()
    y = torch.randn(N) * 0.3

    Ab = A.unsqueeze(0).to(DEV).contiguous()
    yb = y.unsqueeze(0).to(DEV).contiguous()
    rho = torch.tensor([[0.05, 0.01]], device=DEV)
    xg, Yg, Sg, nh = ops.ext().enet_lbfgs_solve(Ab, yb, rho, 20, 10, 7)
    pen = torch.zeros(1, device=DEV)
    EE, reward = ops.ext().enet_influence(Ab, yb, xg, Yg, Sg, nh, pen,
                                          rho)
    torch.cuda.synchronize()

    # CPU oracle on the SAME curvature pairs (from the GPU solve)
    k = int(nh[0])
    Yc = Yg[0, :k].cpu()
    Sc = Sg[0, :k].cpu()
    EE_ref = enet_ops.influence_eigs_reference(A, Yc, Sc, rho1=0.05)
    assert torch.allclose(EE[0].cpu(), EE_ref, rtol=1e-2, atol=1e-3), \
        f"max err {(EE[0].cpu()-EE_ref).abs().max()}"

    x_cpu = xg[0].cpu()
    err = torch.norm(A @ x_cpu - y)
    r_ref = torch.norm(y) / err + EE_ref.min() / EE_ref.max()
    assert abs(float(reward[0]) - float(r_ref)) < 2e-2 * abs(float(r_ref)) + 1e-3


def test_env_gpu_step_end_to_end():
    from smartcal_amd.envs.enet import ENetEnv
    np.random.seed(0)
    torch.manual_seed(0)
    env = ENetEnv(20, 20, device=DEV)
    obs = env.reset()
    obs2, r, done, info = env.step(np.zeros(2, dtype=np.float32))
    assert obs2["eig"].is_cuda
    assert torch.isfinite(r)
    assert torch.isfinite(obs2["eig"]).all()


def test_sac_graphed_learn():
    from smartcal_amd.rl.sac import Agent
    np.random.seed(0)
    torch.manual_seed(0)
    agent = Agent(gamma=0.99, batch_size=8, n_actions=2, tau=0.005,
                  max_mem_size=64, input_dims=[24], lr_a=1e-3, lr_c=1e-3,
                  reward_scale=2, alpha=0.03, device=DEV)
    obs = {"eig": torch.randn(8), "A": torch.randn(16)}
    for _ in range(10):
        a = agent.choose_action(obs)
        obs2 = {"eig": torch.randn(8), "A": torch.randn(16)}
        agent.store_transition(obs, a, 0.5, obs2, False,
                               np.zeros(2, np.float32))
        obs = obs2
    agent.enable_cuda_graph()
    before = agent.actor_fp.flat.clone()
    for _ in range(5):
        agent.learn()
    torch.cuda.synchronize()
    assert agent.learn_counter == 5
    assert torch.isfinite(agent.actor_fp.flat).all()
    assert not torch.allclose(before, agent.actor_fp.flat)
    assert torch.isfinite(agent.critic_1_fp.flat).all()
    # polyak kept targets tracking
    assert torch.isfinite(agent.target_critic_1_fp.flat).all()


def test_sac_agent_gpu_learn():
    from smartcal_amd.rl.sac import Agent
    np.random.seed(0)
    torch.manual_seed(0)
    agent = Agent(gamma=0.99, batch_size=8, n_actions=2, tau=0.005,
                  max_mem_size=64, input_dims=[24], lr_a=1e-3, lr_c=1e-3,
                  reward_scale=2, alpha=0.03, device=DEV)
    obs = {"eig": torch.randn(8), "A": torch.randn(16)}
    for _ in range(10):
        a = agent.choose_action(obs)
        obs2 = {"eig": torch.randn(8), "A": torch.randn(16)}
        agent.store_transition(obs, a, 0.5, obs2, False,
                               np.zeros(2, np.float32))
        agent.learn()
        obs = obs2
    torch.cuda.synchronize()
    assert agent.learn_counter >= 1
    assert torch.isfinite(agent.actor_fp.flat).all()


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_mlp_chain_matches_layers():
    """Chain kernel ≡ per-layer fused path: outputs and all grads."""
    import copy
    from smartcal_amd.ops.linear import FusedLinear, fused_chain
    torch.manual_seed(0)
    layers = torch.nn.ModuleList([
        FusedLinear(420, 512), FusedLinear(512, 256),
        FusedLinear(256, 128)]).cuda()
    layers_ref = copy.deepcopy(layers)
    for B in (1, 64):
        x = torch.randn(B, 420, device="cuda")
        y = fused_chain(x, tuple(layers))
        y_ref = x
        for m in layers_ref:
            y_ref = m(y_ref)
        torch.testing.assert_close(y, y_ref, rtol=2e-4, atol=2e-4)
    # gradients
    for m in (*layers, *layers_ref):
        for p in m.parameters():
            p.grad = None
    x = torch.randn(64, 420, device="cuda", requires_grad=True)
    x2 = x.detach().clone().requires_grad_(True)
    fused_chain(x, tuple(layers)).square().sum().backward()
    yr = x2
    for m in layers_ref:
        yr = m(yr)
    yr.square().sum().backward()
    torch.testing.assert_close(x.grad, x2.grad, rtol=2e-3, atol=2e-3)
    for m, mr in zip(layers, layers_ref):
        for (n, p), (_, pr) in zip(m.named_parameters(),
                                   mr.named_parameters()):
            torch.testing.assert_close(p.grad, pr.grad, rtol=2e-3,
                                       atol=2e-3)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_conv2d_k5s2_matches_torch():
    """Direct-conv HIP kernels ≡ F.conv2d (fwd + dx/dW/db)."""
    from smartcal_amd.ops.conv import conv2d_k5s2
    torch.manual_seed(0)
    for (B, Cin, Cout, H) in ((4, 1, 16, 33), (3, 16, 32, 29),
                              (2, 32, 32, 13)):
        x = torch.randn(B, Cin, H, H, device="cuda", requires_grad=True)
        W = torch.randn(Cout, Cin, 5, 5, device="cuda",
                        requires_grad=True) * 0.1
        W.retain_grad()
        b = torch.randn(Cout, device="cuda", requires_grad=True)
        b.retain_grad()
        x2 = x.detach().clone().requires_grad_(True)
        W2 = W.detach().clone().requires_grad_(True)
        b2 = b.detach().clone().requires_grad_(True)
        y = conv2d_k5s2(x, W, b)
        y2 = F.conv2d(x2, W2, b2, stride=2)
        torch.testing.assert_close(y, y2, rtol=2e-4, atol=2e-4)
        g = torch.randn_like(y)
        y.backward(g)
        y2.backward(g)
        torch.testing.assert_close(x.grad, x2.grad, rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(W.grad, W2.grad, rtol=2e-3, atol=2e-3)
        torch.testing.assert_close(b.grad, b2.grad, rtol=2e-3, atol=2e-3)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_enet_solver_finite_small_rho():
    """Regression: small-rho (ill-conditioned) instances must stay finite.

    A seed-2 hint-path SAC episode drove rho to ~(0.07, 0.06) on an
    instance where the in-kernel two-loop overflowed (1/ys) and the
    unguarded line search emitted NaN x, poisoning the replay buffer.
    The solver now carries the reference's NaN guards
    (`lbfgsnew.py:556,624,673,695`); sweep the degenerate regime and
    assert everything stays finite.
    """
    from smartcal_amd.envs.enet import ENetEnv
    from smartcal_amd.utils.device import seed_everything
    from smartcal_amd import ops

    seed_everything(2)
    env = ENetEnv(20, 20, provide_hint=True)
    env.reset()
    for rho1 in (1e-3, 0.0621, 0.0696, 0.5, 5.0):
        for rho2 in (1e-3, 0.0621, 0.5):
            x, EE, r = ops.enet.solve_and_influence(
                env.A, env.y0, float(rho1), float(rho2), 0.0)
            assert torch.isfinite(x).all(), (rho1, rho2)
            assert torch.isfinite(EE).all(), (rho1, rho2)
            assert np.isfinite(float(r)), (rho1, rho2)
    # and through the env step API (device path) with adversarial actions;
    # the degenerate-pair filter bounds the eigen-ratio reward term, so
    # rewards stay at sane magnitudes (pre-filter failures were ~-4e6)
    obs = env.reset()
    for a in ([-1.0, -1.0], [0.3863, 0.2346], [1.0, 1.0], [-0.99, 0.99]):
        act = torch.tensor(a, device="cuda")
        out = env.step(act)
        r = float(out[1])
        assert np.isfinite(r), a
        assert r > -1e5, (a, r)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_enet_solver_batched_matches_single():
    """The E>1 batch path (one workgroup per env, `enet_solver.hip`
    blockIdx.x) computes exactly what E separate E=1 launches compute —
    per-block work is independent and deterministic."""
    from smartcal_amd import ops
    torch.manual_seed(7)
    E, N, M = 8, 20, 20
    A = torch.randn(E, N, M, device="cuda")
    A = A / A.flatten(1).norm(dim=1).reshape(E, 1, 1)
    y = torch.randn(E, N, device="cuda") * 0.3
    rho = (torch.rand(E, 2, device="cuda") * 0.09 + 0.001)
    pen = torch.zeros(E, device="cuda")
    xb, Yb, Sb, nhb = ops.ext().enet_lbfgs_solve(
        A.contiguous(), y.contiguous(), rho.contiguous(), 20, 10, 7)
    EEb, rb = ops.ext().enet_influence(A.contiguous(), y.contiguous(),
                                       xb, Yb, Sb, nhb, pen,
                                       rho.contiguous())
    for e in range(E):
        x1, Y1, S1, nh1 = ops.ext().enet_lbfgs_solve(
            A[e:e + 1].contiguous(), y[e:e + 1].contiguous(),
            rho[e:e + 1].contiguous(), 20, 10, 7)
        EE1, r1 = ops.ext().enet_influence(
            A[e:e + 1].contiguous(), y[e:e + 1].contiguous(),
            x1, Y1, S1, nh1, pen[e:e + 1], rho[e:e + 1].contiguous())
        assert torch.equal(xb[e], x1[0]), e
        assert torch.equal(EEb[e], EE1[0]), e
        assert torch.equal(rb[e], r1[0]), e


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_vec_enet_env_gpu():
    """Vectorized env steps E problems in one kernel launch."""
    from smartcal_amd.envs.vec_enet import VecENetEnv
    torch.manual_seed(1)
    env = VecENetEnv(16, 20, 20, device=torch.device("cuda"))
    env.reset()
    a = torch.rand(16, 2, device="cuda") * 2 - 1
    obs, r, done, _ = env.step(a)
    assert r.shape == (16,) and torch.isfinite(r).all()
    assert obs["eig"].shape == (16, 20)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_transformer_agent_learn_gpu():
    """Transformer actor/critic SAC learn step on the fused-linear HIP
    kernels (BASELINE.json calibenv transformer config)."""
    from smartcal_amd.rl.sac_cnn import Agent
    torch.manual_seed(0)
    M = 3
    agent = Agent(gamma=0.99, batch_size=4, n_actions=2 * M, tau=0.005,
                  max_mem_size=32, input_dims=(1, 32, 32), M=M,
                  lr_a=1e-3, lr_c=1e-3, arch="transformer",
                  device=torch.device("cuda"))
    s = {"img": torch.rand(1, 32, 32), "sky": torch.rand(7 * (M + 1))}
    a = agent.choose_action(s)
    for _ in range(6):
        agent.store_transition(s, a, 0.5, s, False,
                               np.zeros(2 * M, np.float32))
    agent.learn()
    torch.cuda.synchronize()
    a2 = np.asarray(agent.choose_action(s))
    assert np.isfinite(a2).all()


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_get_hint_batched_matches_cpu_quality():
    """GPU get_hint (one batched 50-solve kernel launch) picks lambdas
    whose CV error is as good as the serial CPU grid search's."""
    from smartcal_amd.envs.enet import ENetEnv, LOW, HIGH
    from smartcal_amd.ops import enet as enet_ops
    torch.manual_seed(5)
    env = ENetEnv(20, 20, provide_hint=True, device=torch.device("cuda"))
    env.reset()
    env._observe_y()
    hint_gpu = env.get_hint()

    env_cpu = ENetEnv.__new__(ENetEnv)
    env_cpu.__dict__.update(env.__dict__)
    env_cpu.device = torch.device("cpu")
    env_cpu.A = env.A.cpu()
    env_cpu.y = env.y.cpu()
    env_cpu.y0 = env.y0.cpu()
    hint_cpu = env_cpu.get_hint()

    def cv_mse(hint):
        lam = hint * (HIGH - LOW) / 2 + (HIGH + LOW) / 2
        l1, l2 = float(lam[0]), float(lam[1])
        A, y = env_cpu.A, env_cpu.y
        n = 10
        tot = 0.0
        for tr, te in ((slice(0, n), slice(n, 20)),
                       (slice(n, 20), slice(0, n))):
            x, _ = enet_ops.lbfgs_solve_reference(A[tr], y[tr], rho1=l2,
                                                  rho2=l1, epochs=5,
                                                  max_iter=10)
            r = A[te] @ x - y[te]
            tot += float((r * r).mean())
        return tot

    assert cv_mse(hint_gpu) <= cv_mse(hint_cpu) * 1.05 + 1e-6


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs GPU')
def test_enet_kernel_kkt_conditions():
    """Approximate KKT optimality of the in-kernel solve across the
    rho range (incl. the small-rho regime the guards target)."""
    from smartcal_amd import ops
    torch.manual_seed(9)
    # (the deep small-rho corner converges more loosely under the
    # epoch early-stops; its safety is covered by the finiteness and
    # reward-magnitude tests above)
    for rho1, rho2 in ((0.05, 0.02), (0.01, 0.005)):
        N = M = 20
        A = torch.randn(N, M, device="cuda")
        A = A / A.norm()
        y = A @ (torch.randn(M, device="cuda")
                 * (torch.rand(M, device="cuda") > 0.5))
        rho = torch.tensor([[rho1, rho2]], device="cuda")
        xg, *_ = ops.ext().enet_lbfgs_solve(
            A.unsqueeze(0).contiguous(), y.unsqueeze(0).contiguous(),
            rho, 20, 10, 7)
        x = xg[0]
        g_smooth = 2 * A.t() @ (A @ x - y) + 2 * rho1 * x
        scale = float(g_smooth.abs().max().clamp(min=1.0))
        on = x.abs() > 1e-3
        if on.any():
            kkt_on = (g_smooth[on] + rho2 * torch.sign(x[on])).abs().max()
            assert float(kkt_on) < 0.08 * scale + 0.03, (rho1, float(kkt_on))
        if (~on).any():
            kkt_off = g_smooth[~on].abs().max()
            assert float(kkt_off) <= rho2 * 2.0 + 0.03, (rho1,
                                                         float(kkt_off))


def test_per_sample_kernel_matches_torch_oracle():
    """per_sample_kernel vs the torch cumsum+searchsorted oracle.

    Integer-valued priorities keep every partial sum exact in fp32 (total
    << 2^24), so the stratified indices must match EXACTLY; probs and
    max-normalized IS weights to fp32 tolerance."""
    from smartcal_amd.ops import per as per_ops
    for n, B in [(7, 4), (64, 64), (1024, 64), (16000, 256), (1, 8)]:
        torch.manual_seed(n + B)
        pri = torch.randint(1, 11, (n,), device=DEV).float()
        pri[torch.rand(n, device=DEV) < 0.2] = 0.0  # zero-priority runs
        if float(pri.sum()) == 0.0:
            pri[0] = 1.0
        u = torch.rand(B, device=DEV)
        beta = 0.62
        idx_g, probs_g, w_g = ops.ext().per_sample(pri, u, beta)
        idx_t, probs_t = per_ops._torch_stratified(pri, B, u)
        w_t = per_ops.importance_weights(probs_t, n, beta)
        assert torch.equal(idx_g, idx_t), (n, B)
        assert torch.allclose(probs_g, probs_t, atol=1e-7)
        assert torch.allclose(w_g, w_t, atol=1e-5, rtol=1e-5)


def test_per_update_kernel_matches_torch():
    from smartcal_amd.ops import per as per_ops
    torch.manual_seed(3)
    n, B = 512, 64
    pri = torch.rand(n, device=DEV) + 0.1
    pri_ref = pri.clone()
    idx = torch.randperm(n, device=DEV)[:B]
    td = torch.randn(B, device=DEV) * 2
    ops.ext().per_update(pri, idx, td.contiguous(), 0.01, 0.6, 1.0)
    ref = (td.abs() + 0.01).clamp(max=1.0).pow(0.6)
    pri_ref[idx] = ref
    assert torch.allclose(pri, pri_ref, atol=1e-6)


def test_per_buffer_gpu_uses_kernel_end_to_end():
    """PERBuffer on GPU: sample indices within range, weights in (0,1],
    priorities updated on device, distribution sane."""
    from smartcal_amd.rl.buffers import PERBuffer
    torch.manual_seed(5)
    buf = PERBuffer(256, [12], 2, device=DEV)
    for i in range(300):
        s = torch.randn(12)
        buf.store_transition(s, torch.randn(2), float(i), s, False,
                             torch.zeros(2))
    (state, act, rew, state_, done, hint), idx, w = buf.sample_buffer(64)
    assert state.shape == (64, 12) and idx.shape == (64,)
    assert idx.min() >= 0 and idx.max() < 256
    assert float(w.max()) <= 1.0 + 1e-6 and float(w.min()) > 0
    buf.update_priorities(idx, torch.randn(64, 1, device=DEV))
    assert torch.isfinite(buf.priorities).all()


def test_fused_linear_bf16_matches_fp32_oracle():
    """bf16-compute fused linear (fp32 master weights, bf16 MFMA) vs the
    fp32 torch oracle: one bf16 rounding per operand => ~1e-2 relative."""
    from smartcal_amd.ops import linear as linear_ops
    torch.manual_seed(0)
    for (B, K, N) in [(64, 420, 512), (64, 512, 256), (3, 33, 17),
                      (64, 128, 4), (20, 7, 64)]:
        x = torch.randn(B, K)
        W = torch.randn(N, K) / K ** 0.5
        b = torch.randn(N)
        g = torch.rand(N) + 0.5
        be = torch.randn(N)
        ref = F.elu(F.layer_norm(F.linear(x, W, b), (N,), g, be))
        y, zhat, rstd = ops.ext().fused_linear_bf16_fwd(
            x.cuda(), W.cuda(), b.cuda(), g.cuda(), be.cuda(),
            linear_ops.ACT_ELU, True)
        err = (y.cpu() - ref).abs().max()
        # LN rescales to unit variance so abs tolerance is meaningful
        assert float(err) < 6e-2, (B, K, N, float(err))


def test_gemm_bf16_kernels_match_fp32():
    torch.manual_seed(1)
    for (M, K, N) in [(64, 512, 420), (64, 64, 256), (17, 33, 65)]:
        A = torch.randn(M, K, device=DEV)
        B = torch.randn(K, N, device=DEV) / K ** 0.5
        C = ops.ext().mfma_gemm_nn_bf16(A, B)
        ref = (A.double() @ B.double()).float()
        scale = ref.abs().max().clamp(min=1.0)
        assert float((C - ref).abs().max() / scale) < 3e-2
    # tn + bias accumulate
    Bb, N, K = 64, 256, 420
    dz = torch.randn(Bb, N, device=DEV)
    x = torch.randn(Bb, K, device=DEV)
    dW = torch.zeros(N, K, device=DEV)
    db = torch.zeros(N, device=DEV)
    ops.ext().mfma_gemm_tn_bias_into_bf16(dz, x, dW, db)
    refW = (dz.double().t() @ x.double()).float()
    refb = dz.sum(0)
    s = refW.abs().max().clamp(min=1.0)
    assert float((dW - refW).abs().max() / s) < 3e-2
    assert torch.allclose(db, refb, atol=1e-3, rtol=1e-4)


def test_bf16_agent_learn_step_finite_and_close():
    """A TD3+PER learn step in bf16 compute mode stays finite and its
    critic outputs track the fp32 mode closely (same seed/weights)."""
    from smartcal_amd.ops import linear as linear_ops
    from smartcal_amd.rl.td3 import Agent
    try:
        results = {}
        for mode in ("fp32", "bf16"):
            linear_ops.set_compute_dtype(mode)
            torch.manual_seed(7)
            np.random.seed(7)
            ag = Agent(gamma=0.99, batch_size=16, n_actions=2, tau=0.005,
                       max_mem_size=64, input_dims=[40], lr_a=1e-3,
                       lr_c=1e-3, warmup=0, noise=0.1, prioritized=True,
                       device=DEV)
            s = torch.randn(24, 40)
            for i in range(24):
                ag.store_transition({"eig": s[i, :20], "A": s[i, 20:]},
                                    np.zeros(2, np.float32), float(i % 3),
                                    {"eig": s[i, :20], "A": s[i, 20:]},
                                    False, np.zeros(2, np.float32))
            for _ in range(4):
                ag.learn()
            q = ag.critic_1(s.cuda(), torch.zeros(24, 2, device=DEV))
            assert torch.isfinite(q).all()
            results[mode] = q.detach().cpu()
        diff = (results["fp32"] - results["bf16"]).abs().max()
        scale = results["fp32"].abs().max().clamp(min=1.0)
        assert float(diff / scale) < 0.15, float(diff)
    finally:
        linear_ops.set_compute_dtype("fp32")


def test_attention_kernel_matches_torch_oracle():
    """Fused attention fwd/bwd vs the torch composition, at both workload
    shapes: heads-as-tokens (T=6, dh=66) and sky tokens (T=22, dh=16)."""
    from smartcal_amd.ops import attention as attn_ops
    torch.manual_seed(0)
    for (G, T, dh) in [(64, 6, 66), (128, 22, 16), (8, 32, 96),
                       (4, 1, 8), (16, 17, 33)]:
        q = torch.randn(G, T, dh, device=DEV, requires_grad=True)
        k = torch.randn(G, T, dh, device=DEV, requires_grad=True)
        v = torch.randn(G, T, dh, device=DEV, requires_grad=True)
        o, a = attn_ops.scaled_dot_product(q, k, v)
        q2 = q.detach().clone().requires_grad_(True)
        k2 = k.detach().clone().requires_grad_(True)
        v2 = v.detach().clone().requires_grad_(True)
        o_ref, a_ref = attn_ops._torch_sdp(q2, k2, v2)
        assert torch.allclose(o, o_ref, atol=2e-5, rtol=1e-4), (T, dh)
        assert torch.allclose(a, a_ref, atol=2e-5, rtol=1e-4)
        do = torch.randn_like(o)
        o.backward(do)
        o_ref.backward(do)
        for g1, g2 in ((q.grad, q2.grad), (k.grad, k2.grad),
                       (v.grad, v2.grad)):
            assert torch.allclose(g1, g2, atol=5e-5, rtol=1e-3), (T, dh)


def test_transformer_models_use_attention_kernel():
    """TransformerEncoder + TokenMHA end-to-end on GPU: forward/backward
    finite and matching the CPU reference model."""
    from smartcal_amd.models.transformer import TransformerEncoder
    from smartcal_amd.rl.transformer_networks import TokenMHA
    torch.manual_seed(1)
    net = TransformerEncoder(num_layers=1, input_dim=6 * (8 * 8 + 8),
                             model_dim=6 * 66, num_classes=5,
                             num_heads=6).cuda()
    x = torch.randn(16, 6 * (8 * 8 + 8), device=DEV)
    y = net(x)
    loss = y.sum()
    loss.backward()
    assert torch.isfinite(y).all() and y.shape == (16, 5)
    mha = TokenMHA(64, 4).cuda()
    t = torch.randn(8, 12, 64, device=DEV, requires_grad=True)
    out = mha(t)
    out.sum().backward()
    assert torch.isfinite(out).all() and t.grad is not None
    assert torch.isfinite(t.grad).all()


def test_two_loop_kernel_matches_torch_oracle():
    """two_loop_apply (one launch, m RHS) vs the torch composition —
    incl. filtered (ro=0) pairs and long vectors."""
    from smartcal_amd import autograd_tools as at_
    torch.manual_seed(0)
    for (h, n, m) in [(7, 20, 20), (5, 4097, 3), (10, 100000, 1)]:
        Y = torch.randn(h, n, device=DEV)
        S = torch.randn(h, n, device=DEV)
        Q = torch.randn(n, m, device=DEV)
        ref = at_.inv_hessian_mult_mat(Y.cpu(), S.cpu(), Q.cpu())
        out = at_.inv_hessian_mult_mat(Y, S, Q)
        scale = ref.abs().max().clamp(min=1.0)
        assert float((out.cpu() - ref).abs().max() / scale) < 1e-4, (h, n)
    # optimizer direction path: GPU LBFGSNew == CPU LBFGSNew trajectory
    from smartcal_amd.optim import LBFGSNew
    A = torch.randn(64, 32)
    b = torch.randn(64)

    def run(device):
        torch.manual_seed(1)
        x = torch.zeros(32, requires_grad=True, device=device)
        Ad, bd = A.to(device), b.to(device)
        opt = LBFGSNew([x], history_size=7, max_iter=10,
                       line_search_fn=True, batch_mode=False)

        def closure():
            if torch.is_grad_enabled():
                opt.zero_grad()
            loss = ((Ad @ x - bd) ** 2).sum()
            if loss.requires_grad:
                loss.backward()
            return loss
        for _ in range(5):
            opt.step(closure)
        return x.detach().cpu()

    xc, xg = run("cpu"), run("cuda")
    assert torch.allclose(xc, xg, atol=1e-3, rtol=1e-3)


def test_bf16_chain_matches_per_layer_bf16():
    """mlp_chain_bf16_fwd (whole chain, one launch) ≡ the per-layer bf16
    path: identical casts and MFMA order, so results match tightly;
    and the bf16-mode fused_chain trains (backward on bf16 GEMMs)."""
    from smartcal_amd.ops import linear as linear_ops
    from smartcal_amd.rl.networks import SACActorMLP
    try:
        linear_ops.set_compute_dtype("bf16")
        torch.manual_seed(0)
        x = torch.randn(64, 420, device=DEV)
        Ws, bs, gs, bes = [], [], [], []
        dims = [420, 512, 256, 128]
        for i in range(3):
            Ws.append(torch.randn(dims[i + 1], dims[i], device=DEV)
                      / dims[i] ** 0.5)
            bs.append(torch.randn(dims[i + 1], device=DEV))
            gs.append(torch.rand(dims[i + 1], device=DEV) + 0.5)
            bes.append(torch.randn(dims[i + 1], device=DEV))
        ys, _, _ = ops.ext().mlp_chain_fwd(x, Ws, bs, gs, bes,
                                           [1, 1, 1], True)
        h = x
        for i in range(3):
            h, _, _ = ops.ext().fused_linear_bf16_fwd(
                h.contiguous(), Ws[i], bs[i], gs[i], bes[i], 1, True)
        assert torch.allclose(ys[-1], h, atol=1e-5, rtol=1e-5)
        # end-to-end: a bf16-mode actor trains through the chain
        torch.manual_seed(1)
        actor = SACActorMLP(420, 2).cuda()
        from smartcal_amd.utils.flatten import FlatParams, FusedAdam
        fp = FlatParams(actor)
        opt = FusedAdam(fp, lr=1e-3)
        a, lp = actor.sample_normal(torch.randn(32, 420, device=DEV))
        (lp.mean()).backward()
        opt.step()
        assert torch.isfinite(fp.flat).all()
    finally:
        linear_ops.set_compute_dtype("fp32")
