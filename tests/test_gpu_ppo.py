"""The fused PPO minibatch loss (nmmo_amd/ppo.py, csrc/ppo.hip) on MI355X against SPEC.md §16.

The yardstick is `reference`: the §16 expressions (those of `DeviceTrainer.train`) in torch on the
CPU with autograd, run in float64. `E_ref` is the error of the same function run in float32
against it, and the fused result must stay within 4 x E_ref (`tests/test_gpu_heads.py::within`,
DESIGN §3.9), for every scalar and, as the max over elements, for each gradient vector. The rule
has no floor, so a branch decided differently in float32 and float64 would make E_ref meaningless:
`near_boundary` marks the rows within 1e-3 (relative) of a branch boundary, the generator redraws
such rows, and every random case first asserts that none is left. `clipfrac` is then an exact count.
"""

import ctypes

import numpy as np
import pytest
import torch

from tests.conftest import gpu_available
from tests.test_gpu_heads import within

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ("newlogprob", "entropy", "newvalue", "old_logprob", "advantages", "returns", "old_values")
SCALARS = ("loss", "pg_loss", "v_loss", "entropy_loss", "old_approx_kl", "approx_kl", "clipfrac", "adv_mean", "adv_std")
PRM = dict(clip_coef=0.1, vf_clip_coef=0.1, ent_coef=0.01, vf_coef=0.5, norm_adv=True, clip_vloss=True)
MARGIN = 1e-3


# ---------------------------------------------------------------- the yardstick
def reference(inp, prm, dtype):
    """SPEC §16 in torch on the CPU: ({scalar name: float}, {input name: float64 gradient})."""
    t = {k: torch.from_numpy(inp[k]).to(dtype) for k in NAMES}
    newlogprob, entropy, newvalue = [t[k].requires_grad_(True) for k in NAMES[:3]]
    mb_advantages, mb_returns, mb_values = t["advantages"], t["returns"], t["old_values"]
    logratio = newlogprob - t["old_logprob"]
    ratio = logratio.exp()
    with torch.no_grad():
        old_approx_kl = (-logratio).mean()
        approx_kl = ((ratio - 1) - logratio).mean()
        clipfrac = ((ratio - 1.0).abs() > prm["clip_coef"]).to(dtype).mean()
    adv_mean, adv_std = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    if prm["norm_adv"]:
        adv_mean, adv_std = mb_advantages.mean(), mb_advantages.std()
        mb_advantages = (mb_advantages - adv_mean) / (adv_std + 1e-8)
    pg_loss1 = -mb_advantages * ratio
    pg_loss2 = -mb_advantages * torch.clamp(ratio, 1 - prm["clip_coef"], 1 + prm["clip_coef"])
    pg_loss = torch.max(pg_loss1, pg_loss2).mean()
    if prm["clip_vloss"]:
        v_loss_unclipped = (newvalue - mb_returns) ** 2
        v_clipped = mb_values + torch.clamp(newvalue - mb_values, -prm["vf_clip_coef"], prm["vf_clip_coef"])
        v_loss_clipped = (v_clipped - mb_returns) ** 2
        v_loss = 0.5 * torch.max(v_loss_unclipped, v_loss_clipped).mean()
    else:
        v_loss = 0.5 * ((newvalue - mb_returns) ** 2).mean()
    entropy_loss = entropy.mean()
    loss = pg_loss - prm["ent_coef"] * entropy_loss + v_loss * prm["vf_coef"]
    loss.backward()
    vals = (loss, pg_loss, v_loss, entropy_loss, old_approx_kl, approx_kl, clipfrac, adv_mean, adv_std)
    return ({k: float(v.detach().double()) for k, v in zip(SCALARS, vals)},
            {k: t[k].grad.double().numpy() for k in NAMES[:3]})


def branches(inp, prm):
    """The float64 quantities the branches of §16 compare, per row."""
    x = {k: inp[k].astype(np.float64) for k in NAMES}
    c, k = prm["clip_coef"], prm["vf_clip_coef"]
    ratio = np.exp(x["newlogprob"] - x["old_logprob"])
    adv = x["advantages"]
    if prm["norm_adv"]:
        adv = (adv - adv.mean()) / (adv.std(ddof=1) + 1e-8)
    p1, p2 = -adv * ratio, -adv * np.clip(ratio, 1 - c, 1 + c)
    d = x["newvalue"] - x["old_values"]
    u = (x["newvalue"] - x["returns"]) ** 2
    cl = (x["old_values"] + np.clip(d, -k, k) - x["returns"]) ** 2
    return dict(ratio=ratio, adv=adv, p1=p1, p2=p2, d=d, u=u, cl=cl)


def near_boundary(inp, prm):
    """Rows within MARGIN (relative) of a branch boundary: ratio against 1 +- clip_coef,
    |newvalue - old_values| against vf_clip_coef, and the two arguments of a `max` being equal
    outside the clip range."""
    b = branches(inp, prm)
    c, k = prm["clip_coef"], prm["vf_clip_coef"]
    close = lambda a, ref: np.abs(a - ref) <= MARGIN * np.abs(ref)  # noqa: E731
    bad = close(b["ratio"], 1 - c) | close(b["ratio"], 1 + c)
    outside = (b["ratio"] < 1 - c) | (b["ratio"] > 1 + c)
    bad |= outside & (np.abs(b["p1"] - b["p2"]) <= MARGIN * np.maximum(np.abs(b["p1"]), np.abs(b["p2"])))
    if prm["clip_vloss"]:
        bad |= close(np.abs(b["d"]), k)
        bad |= (np.abs(b["d"]) > k) & (np.abs(b["u"] - b["cl"]) <= MARGIN * np.maximum(b["u"], b["cl"]))
    return bad


def draw(rng, n, scale, prm):
    old_logprob = -np.abs(rng.standard_normal(n)) * 3.0
    old_values = rng.standard_normal(n)
    return {"old_logprob": old_logprob, "newlogprob": old_logprob + scale * rng.standard_normal(n),
            "entropy": 2.0 + rng.standard_normal(n), "old_values": old_values,
            "newvalue": old_values + 1.5 * prm["vf_clip_coef"] * rng.standard_normal(n),
            "advantages": 0.3 + 2.0 * rng.standard_normal(n), "returns": old_values + 0.3 * rng.standard_normal(n)}


def make_inputs(n, scale, seed, prm):
    """float32 inputs drawn from `seed`; rows that land near a branch boundary are drawn again."""
    rng = np.random.default_rng(seed)
    inp = {k: v.astype(np.float32) for k, v in draw(rng, n, scale, prm).items()}
    for _ in range(20):
        bad = near_boundary(inp, prm)
        if not bad.any():
            break
        new = draw(rng, int(bad.sum()), scale, prm)
        for k in NAMES:
            inp[k][bad] = new[k].astype(np.float32)
    return inp


# ---------------------------------------------------------------- running the kernel
def fused(inp, prm, accum=None, scale_loss=None):
    """(scalars, gradients, loss tensor, stats tensor) of one ppo_loss call + backward."""
    from nmmo_amd.ppo import ppo_loss

    t = {k: (v if torch.is_tensor(v) else torch.from_numpy(v).cuda()) for k, v in inp.items()}
    leaves = [t[k].detach().requires_grad_(True) for k in NAMES[:3]]
    loss, stats = ppo_loss(*leaves, *[t[k] for k in NAMES[3:]], accum=accum, **prm)
    assert loss.shape == () and loss.dtype == torch.float32 and stats.dtype == torch.float32
    assert not stats.requires_grad
    (loss if scale_loss is None else scale_loss * loss).backward()
    s = stats.double().cpu().numpy()
    assert s.shape == (len(SCALARS),) and float(loss.detach()) == s[0]
    return dict(zip(SCALARS, s)), {k: x.grad for k, x in zip(NAMES[:3], leaves)}, loss, stats


def check_against_reference(name, inp, prm):
    want, want_g = reference(inp, prm, torch.float64)
    ref32, ref32_g = reference(inp, prm, torch.float32)
    got, got_g, _, _ = fused(inp, prm)
    for k in SCALARS:
        within(f"{name} {k}", np.array([got[k]]), np.array([want[k]]), np.array([ref32[k]]))
    for k in NAMES[:3]:
        g = got_g[k]
        assert g.dtype == torch.float32 and g.shape == (len(inp[k]),)
        within(f"{name} g_{k}", g.double().cpu().numpy(), want_g[k], ref32_g[k])
    return got, want


SIZES = [2, 63, 64, 65, 1023, 1024, 1025, 4099]
FLAGS = [(na, cv) for na in (True, False) for cv in (True, False)]
RANDOM = ([(n, s, True, True) for n in SIZES for s in (0.01, 1.0)] + [(131072, 1.0, True, True)]
          + [(n, s, na, cv) for n in (65, 1025) for s in (0.01, 1.0) for na, cv in FLAGS[1:]])


# ---------------------------------------------------------------- 1. random cases
@pytest.mark.parametrize("n,scale,norm_adv,clip_vloss", RANDOM)
def test_random_batches_match_float64_autograd(n, scale, norm_adv, clip_vloss):
    prm = dict(PRM, norm_adv=norm_adv, clip_vloss=clip_vloss)
    inp = make_inputs(n, scale, 1000 + n, prm)
    assert not near_boundary(inp, prm).any()  # the input condition of the 4 x E_ref rule
    b = branches(inp, prm)
    lo, hi = 1 - prm["clip_coef"], 1 + prm["clip_coef"]
    if n >= 63:  # the batch exercises every branch
        assert (b["adv"] > 0).any() and (b["adv"] < 0).any()
        inside = ((b["ratio"] >= lo) & (b["ratio"] <= hi)).mean()
        if scale == 1.0:
            assert (b["ratio"] < lo).any() and (b["ratio"] > hi).any() and inside < 0.5
        else:
            assert inside > 0.5
        if clip_vloss:
            assert (b["u"] > b["cl"]).any() and (b["cl"] > b["u"]).any() and (np.abs(b["d"]) <= 0.1).any()
    got, _ = check_against_reference(f"n={n} scale={scale} norm_adv={norm_adv} clip_vloss={clip_vloss}", inp, prm)
    count = int((np.abs(b["ratio"] - 1.0) > prm["clip_coef"]).sum())
    assert got["clipfrac"] == float(np.float32(count / n)) and round(got["clipfrac"] * n) == count


# ---------------------------------------------------------------- 2. exact boundaries
def boundary_case(which):
    n = 65
    prm = dict(PRM)
    inp = make_inputs(n, 1.0, 77, prm)
    if which == "ratio-one-clip-zero":  # ratio == 1 == both clamp bounds: a tie inside the (empty) clip range
        inp["newlogprob"] = inp["old_logprob"].copy()
        prm["clip_coef"] = 0.0
    elif which == "value-on-the-clip":  # newvalue - old_values == +-vf_clip_coef exactly
        prm["vf_clip_coef"] = 0.125
        inp["old_values"][:] = 1.0
        inp["newvalue"][:] = np.where(np.arange(n) % 2 == 0, 1.125, 0.875).astype(np.float32)
    elif which == "zero-advantage":  # both policy terms are 0 whatever the ratio
        prm["norm_adv"] = False
        inp["advantages"][::3] = 0.0
    elif which == "constant-advantages":  # std 0: the normalised advantages are 0 / 1e-8
        inp["advantages"][:] = np.float32(0.3)
    return inp, prm


@pytest.mark.parametrize("which", ["ratio-one-clip-zero", "value-on-the-clip", "zero-advantage", "constant-advantages"])
def test_exact_boundaries_match_float64_autograd(which):
    inp, prm = boundary_case(which)
    got, want = check_against_reference(which, inp, prm)
    _, got_g, _, _ = fused(inp, prm)
    g = {k: v.double().cpu().numpy() for k, v in got_g.items()}
    if which == "ratio-one-clip-zero":
        assert got["clipfrac"] == 0 and got["approx_kl"] == 0 and got["old_approx_kl"] == 0
        assert np.any(g["newlogprob"] != 0)  # the halves of the tie add up to -A ratio / N
    if which == "value-on-the-clip":  # the clamp passes the gradient at its bounds: (v - R) vf_coef / N
        want_gv = prm["vf_coef"] * (inp["newvalue"].astype(np.float64) - inp["returns"]) / len(inp["returns"])
        assert np.array_equal(g["newvalue"], want_gv.astype(np.float32).astype(np.float64))
    if which == "zero-advantage":
        assert np.all(g["newlogprob"][::3] == 0) and np.any(g["newlogprob"] != 0)
    if which == "constant-advantages":
        assert got["adv_std"] == 0 and got["pg_loss"] == 0 and np.all(g["newlogprob"] == 0)
        assert np.isfinite(got["loss"])


# ---------------------------------------------------------------- 3. other properties
def test_same_inputs_give_bit_identical_outputs():
    for n in (1024, 4099):
        inp = make_inputs(n, 1.0, 5, PRM)
        _, g1, l1, s1 = fused(inp, PRM)
        _, g2, l2, s2 = fused(inp, PRM)
        assert torch.equal(l1, l2) and torch.equal(s1, s2)
        for k in NAMES[:3]:
            assert torch.equal(g1[k], g2[k])


def test_a_scaled_loss_scales_the_gradients():
    inp = make_inputs(1025, 1.0, 6, PRM)
    _, g1, _, _ = fused(inp, PRM)
    _, g2, _, _ = fused(inp, PRM, scale_loss=2.0)
    for k in NAMES[:3]:
        assert torch.equal(g2[k], 2.0 * g1[k]) and bool((g1[k] != 0).any())


def test_accumulator_sums_the_calls_stats():
    from nmmo_amd import ppo

    acc = ppo.new_accumulator("cuda")
    total = torch.zeros(ppo.N_STATS, dtype=torch.float64, device="cuda")
    for seed, n in ((1, 1024), (2, 65), (3, 1025)):
        _, _, _, stats = fused(make_inputs(n, 1.0, seed, PRM), PRM, accum=acc)
        total = total + stats[:ppo.N_STATS].double()
    assert torch.equal(acc[:ppo.N_STATS], total)
    assert float(acc[ppo.N_STATS]) == 3.0
    assert bool((acc[:ppo.N_STATS] != 0).all())


def test_non_contiguous_inputs_are_handled():
    inp = make_inputs(1025, 1.0, 7, PRM)
    _, g1, l1, s1 = fused(inp, PRM)
    strided = {}
    for k, v in inp.items():
        wide = torch.full((len(v), 3), float("nan"), dtype=torch.float32, device="cuda")
        wide[:, 1] = torch.from_numpy(v).cuda()
        strided[k] = wide[:, 1]
        assert not strided[k].is_contiguous()
    _, g2, l2, s2 = fused(strided, PRM)
    assert torch.equal(l1, l2) and torch.equal(s1, s2)
    for k in NAMES[:3]:
        assert torch.equal(g1[k], g2[k])


def test_runs_on_the_current_stream():
    inp = make_inputs(1024, 1.0, 8, PRM)
    _, g1, l1, s1 = fused(inp, PRM)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        _, g2, l2, s2 = fused(inp, PRM)
    side.synchronize()
    assert torch.equal(s1, s2) and torch.equal(g1["newvalue"], g2["newvalue"])


@pytest.mark.parametrize("n", [65, 1024, 1025])
def test_outputs_do_not_write_past_n(n):
    """nmp_loss itself, into NaN-filled buffers with guard elements on both sides of every output:
    every entry of the outputs is stored (no pre-zeroing by the caller), no guard is touched."""
    from nmmo_amd import ppo

    G = 64
    inp = make_inputs(n, 1.0, 9, PRM)
    dev = [torch.from_numpy(inp[k]).cuda() for k in NAMES]
    sizes = [1, ppo.N_OUT, n, n, n]  # loss, stats, g_newlogprob, g_entropy, g_newvalue
    bufs = [torch.full((G + s + G,), float("nan"), dtype=torch.float32, device="cuda") for s in sizes]
    params = ppo.params_struct(**PRM)
    rc = ppo.lib().nmp_loss(ctypes.byref(params), n, *[t.data_ptr() for t in dev],
                            *[b.data_ptr() + 4 * G for b in bufs], None, torch.cuda.current_stream().cuda_stream)
    ppo.check(rc, "nmp_loss")
    torch.cuda.synchronize()
    for b, s in zip(bufs, sizes):
        host = b.cpu().numpy()
        assert np.isnan(host[:G]).all() and np.isnan(host[G + s:]).all()
        assert not np.isnan(host[G:G + s]).any()
    _, g, loss, stats = fused(inp, PRM)
    assert torch.equal(bufs[0][G:G + 1], loss.reshape(1)) and torch.equal(bufs[1][G:G + ppo.N_OUT], stats)
    for b, k in zip(bufs[2:], NAMES[:3]):
        assert torch.equal(b[G:G + n], g[k])
