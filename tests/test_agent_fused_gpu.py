"""Fused agent-branch kernels (csrc/agent_fused.hip: stj_agent_pack / stj_agent_enc_* / stj_agent_int_*) against (a) the float64
restatement of trajNet.py:29-48,65-87,125-187 (oracle/torch_ref._traj, handed the Dropout masks the kernels drew) and (b) the
layer-by-layer HIP chain they replace (model.fused_agent = False) with the SAME draws: the branch's output (agent keys + mask) and the
gradient of every traj_net/* parameter."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

VERBOSE = False
CFG = dict(input_size=(128, 128), window_size=8, embed_dim=96, depths=[2, 2, 2], num_heads=[3, 6, 12])


def _tracks(B, seed, n_obs=48, n_occ=16, empty_scene=False):
    g = torch.Generator().manual_seed(seed)

    def agents(n):
        a = torch.zeros((B, n, 11, 8))
        a[..., 0:2] = torch.rand((B, n, 11, 2), generator=g) * 8 - 4
        a[..., 2:4] = torch.randn((B, n, 11, 2), generator=g)
        a[..., 4] = torch.rand((B, n, 11), generator=g) * 6.283 - 3.1416
        ty = torch.randint(0, 3, (B, n), generator=g)
        for k in range(3):
            a[..., 5 + k] = (ty == k).float()[..., None]
        # ONE invalid step (x == 0) in half of the tracks, and padded (all-zero) agents.  (Two invalid steps of one track attend
        # uniformly, i.e. produce bitwise-equal rows in front of the max-pool: an exact tie that TF's reduce_max gradient -- and the
        # kernels -- split evenly, while float64 autograd on BLAS products breaks it by 1e-16 noise: not a case a comparison can use.)
        t0 = torch.randint(0, 11, (B, n), generator=g)
        hit = (torch.arange(11)[None, None] == t0[..., None]) & (torch.rand((B, n, 1), generator=g) < 0.5)
        a[..., 0] = torch.where(hit, torch.zeros(()), a[..., 0])
        a[:, n - n // 4:] = 0
        return a
    obs, occ = agents(n_obs), agents(n_occ)
    if empty_scene:
        obs[0], occ[0] = 0, 0                       # a scene without agents: every logit masked, uniform attention
    return obs.cuda(), occ.cuda()


def _model(dtype, seed=5):
    from strajnet_amd import STrajNet
    model = STrajNet(CFG, fg_msa=True, fg=True, large_ogm=False, dtype=dtype, device='cuda:0', seed=seed)
    torch.manual_seed(seed)
    with torch.no_grad():       # non-trivial biases / LayerNorm parameters (the reference initialises them to 0 / 1)
        for n, p in model.params.items():
            if n.startswith('traj_net/') and n.rsplit('/', 1)[-1] in ('bias', 'gamma', 'beta', 'projection_bias'):
                p.master.add_(0.1 * torch.randn_like(p.master))
    return model


def _run(model, obs, occ, G, training, fused):
    from strajnet_amd import ops
    model.fused_agent = fused
    model.zero_grad()
    model._parts.zero_()
    ops.use_arena(model._arena)
    model._sync_compute_weights()
    model._agent_pack_stale = True
    model._dctx = None
    if training:                      # same state, same site numbering -> the same draws in every run
        model.dropctx.n, model.dropctx.sites = 0, {}
        model._dctx = model.dropctx
    key, cmi = model._traj_net(obs, occ)
    (key.float() * G).sum().backward()
    model._fold_partials()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu().clone() for n, p in model.params.items() if n.startswith('traj_net/')}
    return key.detach().double().cpu(), cmi.cpu(), grads


def _ref(model, obs, occ, G, training, B):
    from oracle import torch_ref
    from oracle.masks import masks_from_model
    W = {n: p.master.detach().double().cpu().requires_grad_(n.startswith('traj_net/')) for n, p in model.params.items()}
    torch_ref._MASKS = None
    if training:
        torch_ref._MASKS = {k: torch.as_tensor(v) for k, v in masks_from_model(model, B).items() if k.startswith('traj_net/')}
    try:
        key, cm = torch_ref._traj(W, obs.double().cpu(), occ.double().cpu())
    finally:
        torch_ref._MASKS = None
    (key * G.double().cpu()).sum().backward()
    return key.detach(), cm, {n: (w.grad if w.grad is not None else torch.zeros_like(w)) for n, w in W.items() if n.startswith('traj_net/')}


def _rel(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-30))


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize('training', [False, True])
def test_agent_branch_fused_vs_f64_and_layerwise(dtype, training):
    B = 3
    model = _model(dtype)
    model.dropctx.begin()
    obs, occ = _tracks(B, 11, empty_scene=True)
    G = torch.randn((B, 64, 384), generator=torch.Generator().manual_seed(2)).cuda()
    kf, cf, gf = _run(model, obs, occ, G, training, True)
    kr, cr, gr = _ref(model, obs, occ, G, training, B)
    kl, cl, gl = _run(model, obs, occ, G, training, False)
    assert torch.equal(cf.bool(), cr) and torch.equal(cf, cl)
    f32 = dtype == torch.float32
    # bf16: the two 11-step attention kernels' gradients are small differences of softmax-weighted terms (0.1-0.16 of float64 on the layer-by-layer
    # chain as well): the ceiling is loose there, the bound that bites is "no further from float64 than the chain the kernels replace"
    tol_y, tol_g = (2e-5, 3e-4) if f32 else (2.5e-2, 0.25)
    ef, el = _rel(kf, kr), _rel(kl, kr)
    print(f'{dtype} training={training}: output fused {ef:.2e} layerwise {el:.2e} of f64')
    assert ef < tol_y and ef < 1.5 * el + (1e-6 if f32 else 2e-3), (ef, el)
    worst = 0.0
    for n in (gr if VERBOSE else ()):
        print(f'    {n:60s} fused {_rel(gf[n], gr[n]):.2e} layerwise {_rel(gl[n], gr[n]):.2e} fused-vs-layerwise {_rel(gf[n], gl[n]):.2e}')
    for n in gr:
        e_f, e_l = _rel(gf[n], gr[n]), _rel(gl[n], gr[n])
        worst = max(worst, e_f)
        # never (much) further from float64 than the layer-by-layer chain it replaces
        assert e_f < tol_g and e_f < (2.0 * e_l + 5e-6 if f32 else 1.25 * e_l + 6e-3), (n, e_f, e_l)
    print(f'  worst parameter gradient {worst:.2e}')
    assert len(gr) >= 25
