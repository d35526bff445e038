"""GPU tests of the learn step's MLP path: the one-kernel critic, the actor
chain with its head folded in, the no-grad forwards, the pipelined chain
kernel against a golden recorded before it was pipelined, and the single
launch dW + db GEMM. The one-kernel paths keep every output element's
arithmetic, so every comparison is bit for bit (torch.equal)."""

import hashlib
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    import smartcal_amd.ops as ops
    DEV = torch.device("cuda:0")
else:
    DEV = None

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "chain_fwd_golden.npz"


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert ops.have_hip(), "HIP extension must be loaded on a GPU box"


@pytest.fixture
def composition():
    """Context switch: `with composition(True):` forces the composed
    forwards; always restored."""
    from smartcal_amd.rl import networks

    class _Force:
        def __init__(self, on):
            self.on = on

        def __enter__(self):
            networks.FORCE_COMPOSITION = self.on

        def __exit__(self, *exc):
            networks.FORCE_COMPOSITION = False

    yield _Force
    networks.FORCE_COMPOSITION = False


def _randomise(net, seed):
    """Give LayerNorm affine parameters and heads generic values (the
    initial ones/zeros/0.003 would hide errors)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("ln_weight"):
                p.copy_((torch.rand(p.shape, generator=g) + 0.5).to(p.device))
            elif name.endswith("ln_bias"):
                p.copy_((torch.randn(p.shape, generator=g) * 0.1)
                        .to(p.device))
            elif name.startswith("head."):
                p.copy_((torch.randn(p.shape, generator=g) * 0.1)
                        .to(p.device))
    return net


def _critic(input_dim, seed=0):
    from smartcal_amd.rl.networks import CriticMLP
    torch.manual_seed(seed)
    return _randomise(CriticMLP(input_dim, 2).to(DEV), seed + 1)


def _layer_lists(layers):
    return ([m.weight for m in layers], [m.bias for m in layers],
            [m.ln_weight for m in layers], [m.ln_bias for m in layers])


# ---- 1. fused critic forward against the composition ----------------------

@pytest.mark.parametrize("input_dim", [37, 420])
@pytest.mark.parametrize("B", [1, 16, 17, 64])
def test_critic_forward_matches_composition(input_dim, B):
    net = _critic(input_dim)
    g = torch.Generator().manual_seed(B * 1000 + input_dim)
    state = torch.randn(B, input_dim, generator=g).to(DEV)
    action = (torch.rand(B, 2, generator=g) * 2 - 1).to(DEV)
    e = ops.ext()
    layers = (net.s1, net.s2, net.a1, net.a2, net.head)
    Ws, bs, gs, bes = _layer_lists(layers)
    acts = [1, 1, 1, 1, 0]
    with torch.no_grad():
        q, zcat, ys, zhats, rstds = e.critic_fwd(state, action, Ws, bs, gs,
                                                 bes, acts, True)
        sy, sz, sr = e.mlp_chain_fwd(state, Ws[0:2], bs[0:2], gs[0:2],
                                     bes[0:2], [1, 1], False)
        ay, az, ar = e.mlp_chain_fwd(action, Ws[2:4], bs[2:4], gs[2:4],
                                     bes[2:4], [1, 1], False)
        zc = torch.cat((sy[1], ay[1]), dim=-1).contiguous()
        qc, _, _ = e.fused_linear_fwd(zc, Ws[4], bs[4], None, None, 0, False)
    for l, (y, zh, rs) in enumerate(zip(sy + ay, sz + az, sr + ar)):
        assert torch.equal(ys[l], y), f"y of layer {l}"
        assert torch.equal(zhats[l], zh), f"zhat of layer {l}"
        assert torch.equal(rstds[l], rs), f"rstd of layer {l}"
    assert torch.equal(zcat, zc)
    assert q.shape == (B, 1)
    assert torch.equal(q, qc)


# ---- 2. fused critic backward against the composition ---------------------

@pytest.mark.parametrize("frozen", [False, True])
def test_critic_backward_matches_composition(frozen, composition):
    B, input_dim = 17, 37
    g = torch.Generator().manual_seed(5)
    state = torch.randn(B, input_dim, generator=g).to(DEV)
    action0 = torch.rand(B, 2, generator=g) * 2 - 1
    wq = torch.randn(B, 1, generator=g).to(DEV)
    res = []
    for forced in (False, True):
        net = _critic(input_dim)
        for p in net.parameters():
            p.requires_grad_(not frozen)
        action = action0.clone().to(DEV).requires_grad_(True)
        with composition(forced):
            q = net(state, action)
            (q * wq).sum().backward()
        res.append((q.detach(), action.grad,
                    {n: p.grad for n, p in net.named_parameters()}))
    (q_f, da_f, g_f), (q_c, da_c, g_c) = res
    assert torch.equal(q_f, q_c)
    assert da_f is not None and torch.equal(da_f, da_c)
    assert float(da_f.abs().max()) > 0
    for n in g_c:
        if frozen:
            assert g_f[n] is None and g_c[n] is None, n
        else:
            assert float(g_c[n].abs().max()) > 0, n
            assert torch.equal(g_f[n], g_c[n]), n


# ---- 3. actor chain with folded head against chain + fused_linear ---------

@pytest.mark.parametrize("kind", ["sac", "det"])
@pytest.mark.parametrize("K0", [70, 420])
@pytest.mark.parametrize("B", [1, 17])
def test_actor_folded_head_matches_composition(kind, K0, B, composition):
    from smartcal_amd.rl.networks import DeterministicActorMLP, SACActorMLP
    g = torch.Generator().manual_seed(K0 + B)
    x0 = torch.randn(B, K0, generator=g)
    res = []
    for forced in (False, True):
        torch.manual_seed(2)
        # sac: head 128 -> 4, no activation; det: head 128 -> 1, tanh
        net = SACActorMLP(K0, 2) if kind == "sac" \
            else DeterministicActorMLP(K0, 1)
        net = _randomise(net.to(DEV), 3)
        x = x0.clone().to(DEV).requires_grad_(True)
        with composition(forced):
            out = net(x)
            out = torch.cat(out, dim=-1) if kind == "sac" else out
            w = torch.arange(1, out.shape[-1] + 1, device=DEV).float()
            (out * w).sum().backward()
        res.append((out.detach(), x.grad,
                    {n: p.grad for n, p in net.named_parameters()}))
    (o_f, dx_f, g_f), (o_c, dx_c, g_c) = res
    assert o_f.shape == (B, 4 if kind == "sac" else 1)
    assert torch.equal(o_f, o_c)
    assert torch.equal(dx_f, dx_c)
    for n in g_c:
        assert float(g_c[n].abs().max()) > 0, n
        assert torch.equal(g_f[n], g_c[n]), n


def test_head_backward_identity_matches_kernel():
    """A head without LayerNorm and activation passes dy on as dz; the
    kernel it no longer launches computed dy * 1."""
    g = torch.Generator().manual_seed(0)
    dy = torch.randn(17, 4, generator=g).to(DEV)
    y = torch.randn(17, 4, generator=g).to(DEV)
    empty = torch.empty(0, device=DEV)
    dz, _, _ = ops.ext().fused_linear_bwd_dz(dy, y, empty, empty, None, 0,
                                             False)
    assert torch.equal(dz, dy)


# ---- 4. no-grad mode ------------------------------------------------------

def test_no_grad_forward_stores_only_the_output():
    from smartcal_amd.rl.networks import SACActorMLP
    B, K0 = 17, 70
    g = torch.Generator().manual_seed(9)
    state = torch.randn(B, K0, generator=g).to(DEV)
    action = (torch.rand(B, 2, generator=g) * 2 - 1).to(DEV)
    critic = _critic(K0)
    torch.manual_seed(4)
    actor = _randomise(SACActorMLP(K0, 2).to(DEV), 6)
    q_grad = critic(state, action)
    mu_grad, ls_grad = actor(state)
    assert q_grad.requires_grad and mu_grad.requires_grad
    with torch.no_grad():
        q = critic(state, action)
        mu, ls = actor(state)
    assert not q.requires_grad
    assert torch.equal(q, q_grad.detach())
    assert torch.equal(mu, mu_grad.detach())
    assert torch.equal(ls, ls_grad.detach())
    # the bindings themselves: nothing but the final output comes back
    e = ops.ext()
    Ws, bs, gs, bes = _layer_lists((critic.s1, critic.s2, critic.a1,
                                    critic.a2, critic.head))
    with torch.no_grad():
        q2, zcat, ys, zhats, rstds = e.critic_fwd(
            state, action, Ws, bs, gs, bes, [1, 1, 1, 1, 0], False)
        cy, cz, cr = e.mlp_chain_fwd(state, Ws[0:2], bs[0:2], gs[0:2],
                                     bes[0:2], [1, 1], False, False)
        full, _, _ = e.mlp_chain_fwd(state, Ws[0:2], bs[0:2], gs[0:2],
                                     bes[0:2], [1, 1], False, True)
    assert torch.equal(q2, q)
    assert zcat.numel() == 0 and ys == [] and zhats == [] and rstds == []
    assert len(cy) == 1 and cz == [] and cr == []
    assert torch.equal(cy[0], full[1])


# ---- 5. pipelined chain against the recorded golden -----------------------

def _recorder():
    spec = importlib.util.spec_from_file_location(
        "record_chain_golden", ROOT / "scripts" / "record_chain_golden.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_chain_matches_recorded_golden():
    rec = _recorder()
    gold = np.load(GOLDEN)
    assert len(rec.CHAINS) == 3
    for dims in rec.CHAINS:
        x, layers = rec.make_inputs(dims)
        name = rec.chain_name(dims)
        assert x.shape[0] == 17
        # a different input generator fails here; it never skips
        assert rec.input_digest(x, layers) == str(gold[f"{name}/sha256"]), \
            f"inputs of chain {name} differ from the recorded ones"
        ys, zhats, rstds = rec.run_chain(ops.ext(), x, layers, DEV)
        for l in range(len(layers)):
            for key, got in (("y", ys[l]), ("zhat", zhats[l]),
                             ("rstd", rstds[l])):
                want = torch.from_numpy(gold[f"{name}/{key}{l}"])
                assert torch.equal(got.cpu(), want), f"{name} {key}{l}"


def test_input_digest_is_sha256_of_the_bytes():
    rec = _recorder()
    x, layers = rec.make_inputs((2, 3))
    h = hashlib.sha256(x.numpy().tobytes())
    for t in layers[0]:
        h.update(t.numpy().tobytes())
    assert rec.input_digest(x, layers) == h.hexdigest()


# ---- 6. dW + db in one launch against the two-launch oracle ---------------

@pytest.mark.parametrize("B,N,K", [(17, 40, 70), (64, 1, 320),
                                   (64, 512, 420)])
def test_gemm_tn_bias_into_matches_two_launches(B, N, K):
    g = torch.Generator().manual_seed(B + N + K)
    dz = torch.randn(B, N, generator=g).to(DEV)
    x = torch.randn(B, K, generator=g).to(DEV)
    dW_ref, db_ref = ops.ext().mfma_gemm_tn_bias(dz, x)
    dW = torch.zeros(N, K, device=DEV)
    db = torch.zeros(N, device=DEV)
    ops.ext().mfma_gemm_tn_bias_into(dz, x, dW, db)
    assert torch.equal(dW, dW_ref)
    assert torch.equal(db, db_ref)
    assert float(db.abs().max()) > 0


# ---- 7. a SAC agent, fused against the forced composition -----------------

def _sac_pools(forced, graphed, composition):
    from smartcal_amd.rl.sac import Agent
    np.random.seed(0)
    torch.manual_seed(0)
    with composition(forced):
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
            agent.store_transition(obs, a, 0.25 * (i % 3), obs2, False,
                                   np.zeros(2, np.float32))
            obs = obs2
        if graphed:
            agent.enable_cuda_graph()
        for _ in range(3):
            agent.learn()
        torch.cuda.synchronize()
    assert agent.learn_counter == 3
    return [fp.flat.clone() for fp in (
        agent.actor_fp, agent.critic_1_fp, agent.critic_2_fp,
        agent.target_critic_1_fp, agent.target_critic_2_fp)]


@pytest.mark.parametrize("graphed", [False, True])
def test_sac_learn_matches_composition(graphed, composition):
    """Three learn steps from one seed: the five flat parameter pools of the
    one-kernel path (eager, and captured into a hipGraph) equal those of
    the forced composition run the same way."""
    fused = _sac_pools(False, graphed, composition)
    comp = _sac_pools(True, graphed, composition)
    for i, (a, b) in enumerate(zip(fused, comp)):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), f"pool {i}"
