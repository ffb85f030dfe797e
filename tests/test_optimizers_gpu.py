"""The Adam-family / RMSprop / RAdam kernels of csrc/optim.hip (ffm_optim_step, ffm_optim_step_dev) and everything built on
them: engine.optim_step, the captured step with an optimizer, the trainer's OPTIM.NAME / LR_SCHEDULER surface.

THE BOUND comes from the reference, not from the code under test.  Every comparison has three runs of the same update on
the same inputs: the kernel, torch.optim.<class> on the CPU in float32, and the same class in float64.  A figure is
max |x - x64| / max |x64| over the whole vector, for the parameter UPDATE x = p - p0 and for each state row; the kernel's
figure must not exceed TWICE torch's own float32 figure.  (The factor 2 covers a different but equally valid association of
the same operations.)  The maximum is taken over the vector, never element by element: where g + wd*p nearly cancels,
torch's own float32 run is 1e-3 of lr off as well.

The bound is the issue's, with no floor under it.  The one case it does not define is a torch figure of exactly 0 (a row
both float32 and float64 leave exact, such as amsgrad's running maximum when it does not move; a single element whose
rounding happened to be exact): there the kernel may be off by at most one float32 half-ulp at the scale of the tensor
(2^-24 for a state row, 2^-24 max |p64| / max |update64| for the update, the rounding of p itself).

What makes the bound hold at EVERY size, one element included, is that the kernel follows torch's own float32 association
operation for operation (csrc/optim.hip, optim_update), so its state rows carry torch's roundings; only the device's
correctly rounded sqrt / division against the host's vector library and the double scalars (running products against pow)
can still differ.

Input distribution of the kernel-parity test: every tensor keeps its magnitudes inside one binade (cpu_inputs), so that
many elements stand at the scale of the maximum and the figure is a statement about the vector, not about its two or
three largest entries.  The engine and trainer tests run on real gradients, whose moments are heavy-tailed; as the issue
asks, they bound the parameters only and print the moments' figures.

tests/golden/optim.npz holds parameter trajectories recorded from the reference's build_optimizer for all six optimizers
(make_golden_optim.py): the kernel's distance from a float64 run of the same class must be within the same factor 2 of the
RECORDED float32 trajectory's distance.  For RAdam, whose class lives in the reference only, the float64 run is the
restatement `radam64` below.

Entry points agree BIT for bit (eager, gated on a good step, _dev), and the device-resident step count / powers equal the
host's running products bit for bit.
"""
import json
import os
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from fairfedmed_amd import _lib as L
from fairfedmed_amd import config as C
from fairfedmed_amd import ops, synth
from fairfedmed_amd import optim as O
from fairfedmed_amd.engine import FlatParams

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
GRID_CAP = 2048 * 256
VITB_N = FlatParams(C.vit_b16(rank=8, num_groups=3), "cpu").numel
SIZES = [1, 255, 257, GRID_CAP - 1, GRID_CAP + 1, VITB_N]
LR = 1e-2
HALF_ULP = 2.0 ** -24
KINDS = ["adam", "amsgrad", "adamw", "rmsprop"]
ALL_KINDS = ["sgd", "adam", "adamw", "amsgrad", "rmsprop", "radam"]


# ------------------------------------------------------------------------------------------------------- helpers ---
def cpu_inputs(n, seed, rows, later):
    """p0, g and (for a later step) state rows that a run of the optimizer could have left.  Every tensor keeps its
    magnitudes inside ONE binade (random signs): a figure of the form max |error| / max |value| only says something when
    many elements stand at the scale of the maximum - with normal g, the two or three largest g^2 alone would decide the
    kernel's figure and torch's, and their ratio would be a coin toss at any size."""
    gen = torch.Generator().manual_seed(seed)

    def binade(lo, signed=True):
        x = lo * (1 + torch.rand(n, generator=gen))
        return x * (torch.randint(0, 2, (n,), generator=gen) * 2 - 1) if signed else x

    p0, g = binade(0.5), binade(0.5)
    st = torch.zeros(rows, n)
    if later:
        st[0] = binade(0.25)                          # m (rmsprop: the momentum buffer)
        if rows > 1:
            st[1] = binade(0.5, signed=False)         # v > 0
        if rows > 2:
            st[2] = st[1] * (1 + 0.2 * torch.rand(n, generator=gen))          # vmax >= v
    return p0, g, st


def torch_optimizer(kind, q, lr, spec):
    kw = dict(lr=lr, weight_decay=spec.weight_decay)
    if kind == "rmsprop":
        return torch.optim.RMSprop([q], momentum=spec.momentum, alpha=spec.alpha, **kw)
    if kind == "adamw":
        return torch.optim.AdamW([q], betas=(spec.beta1, spec.beta2), **kw)
    if kind == "sgd":
        return torch.optim.SGD([q], momentum=spec.momentum, **kw)
    return torch.optim.Adam([q], betas=(spec.beta1, spec.beta2), amsgrad=kind == "amsgrad", **kw)


STATE_KEYS = {"rmsprop": ["momentum_buffer", "square_avg"], "adam": ["exp_avg", "exp_avg_sq"], "adamw": ["exp_avg", "exp_avg_sq"],
              "amsgrad": ["exp_avg", "exp_avg_sq", "max_exp_avg_sq"], "sgd": ["momentum_buffer"]}


class TorchRun:
    """torch.optim.<class> on the CPU in `dtype`, optionally seeded at step t0 with given state rows."""

    def __init__(self, kind, p0, spec, lr, dtype, st=None, t0=0):
        self.kind, self.dtype = kind, dtype
        self.q = p0.to(dtype).clone().requires_grad_(True)
        self.opt = torch_optimizer(kind, self.q, lr, spec)
        if t0 > 0:
            state = {k: st[i].to(dtype).clone() for i, k in enumerate(STATE_KEYS[kind])}
            if kind != "sgd":
                state["step"] = torch.tensor(float(t0))
            self.opt.state[self.q] = state

    def step(self, g, repeats, lr=None):
        if lr is not None:
            self.opt.param_groups[0]["lr"] = lr
        self.q.grad = g.to(self.dtype).clone()
        for _ in range(repeats):
            self.opt.step()
        return self

    @property
    def p(self):
        return self.q.detach()

    def rows(self):
        s = self.opt.state[self.q]
        return [s[k] for k in STATE_KEYS[self.kind] if s.get(k) is not None]


def fig(x, x64):
    return float((x.double() - x64).abs().max() / x64.abs().max().clamp_min(1e-300))


def check_bound(what, p_k, rows_k, p0, r32, r64, rows=True):
    """The factor-2 bound of the module docstring on the update and on every state row; returns the measured factors."""
    u64 = r64.p - p0.double()
    e_k, e_t = fig(p_k.double() - p0.double(), u64), fig(r32.p.double() - p0.double(), u64)
    exact = HALF_ULP * float(r64.p.abs().max() / u64.abs().max().clamp_min(1e-300))       # only where torch's figure is 0
    out = {"update": (e_k, e_t)}
    print(f"{what}: update kernel {e_k:.3e} torch32 {e_t:.3e}", end="")
    assert e_k <= (2 * e_t if e_t > 0 else exact), f"{what}: update error {e_k:.3e} > 2 x torch's float32 {e_t:.3e}"
    for i, (a, b32, b64) in enumerate(zip(rows_k, r32.rows(), r64.rows())):
        e_k, e_t = fig(a, b64), fig(b32, b64)
        out[f"row{i}"] = (e_k, e_t)
        print(f" | row{i} kernel {e_k:.3e} torch32 {e_t:.3e}", end="")
        assert not rows or e_k <= (2 * e_t if e_t > 0 else HALF_ULP), \
            f"{what}: state row {i} error {e_k:.3e} > 2 x torch's float32 {e_t:.3e}"
    print()
    return out


def good_state(scale=1024.0):
    return torch.tensor([scale, 1.0 / scale, 1.0, 0.0, 0.0, 65536.0, 2000.0, 1.0], device="cuda")


def dev_desc(spec, lr, steps):
    return torch.tensor(spec.desc_values(lr, steps), dtype=torch.float64, device="cuda")


def run_entry(entry, kind, p, g, state, spec, lr, t0, repeats, scale_state=None, desc=None):
    """One call of an entry point, in place on p / state (GPU tensors); returns the device descriptor for `dev`."""
    if entry == "eager":
        ops.optim_step(p, g, state, kind, spec.desc(lr, t0), repeats)
    elif entry == "gated":
        ops.optim_step(p, g, state, kind, spec.desc(lr, t0), repeats, good_state() if scale_state is None else scale_state)
    else:
        desc = dev_desc(spec, lr, t0) if desc is None else desc
        ops.optim_step_dev(p, g, state, kind, desc, repeats, scale_state)
    return desc


def bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------- kernel parity ---
@pytest.mark.parametrize("later", [False, True], ids=["first", "later"])
@pytest.mark.parametrize("wd", [0.0, 5e-4], ids=["wd0", "wd5e-4"])
@pytest.mark.parametrize("repeats", [1, 2, 16])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_kernel_against_torch_float32_and_float64(kind, n, repeats, wd, later):
    """Every entry point (eager, gated on a good step, _dev) against torch.optim.<class> in float32 and in float64."""
    spec = O.OptimSpec(kind=kind, weight_decay=wd)
    t0 = 10 if later else 0
    p0, g, st = cpu_inputs(n, seed=n % 1000 + 7 * repeats + 3 * later, rows=spec.rows, later=later)
    r32 = TorchRun(kind, p0, spec, LR, torch.float32, st, t0).step(g, repeats)
    r64 = TorchRun(kind, p0, spec, LR, torch.float64, st, t0).step(g, repeats)
    for entry in ("eager", "gated", "dev"):
        p, state = p0.cuda(), st.cuda().contiguous()
        run_entry(entry, kind, p, g.cuda(), state, spec, LR, t0, repeats)
        torch.cuda.synchronize()
        check_bound(f"{kind}/{entry} n={n} x{repeats} wd={wd} t0={t0}", p.cpu(), list(state.cpu()), p0, r32, r64)


def test_unaligned_buffers_take_the_scalar_path_and_agree_bit_for_bit():
    """Rows that do not start on 16 bytes (n not a multiple of 4 with K > 1, or an offset view) run element by element and
    give the bits of the vector path on the same values: the result does not depend on the launch geometry."""
    spec = O.OptimSpec(kind="amsgrad")
    n = 4 * 1000
    p0, g, st = cpu_inputs(n + 1, seed=5, rows=3, later=True)
    pa, ga, sa = p0[:n].cuda().contiguous(), g[:n].cuda().contiguous(), st[:, :n].cuda().contiguous()
    ops.optim_step(pa, ga, sa, "amsgrad", spec.desc(LR, 10), 2)
    pool_p, pool_g = torch.zeros(n + 1, device="cuda"), torch.zeros(n + 1, device="cuda")
    pb, gb = pool_p[1:], pool_g[1:]                   # 4 bytes past a 16-byte boundary
    pb.copy_(p0[:n]), gb.copy_(g[:n])
    sb = st[:, :n].cuda().contiguous()
    ops.optim_step(pb, gb, sb, "amsgrad", spec.desc(LR, 10), 2)
    assert bits_equal(pa, pb.contiguous()) and bits_equal(sa, sb)
    m = n - 1                                         # n % 4 != 0: rows 1, 2 are unaligned
    pc, gc, sc = p0[:m].cuda().contiguous(), g[:m].cuda().contiguous(), st[:, :m].cuda().contiguous()
    ops.optim_step(pc, gc, sc, "amsgrad", spec.desc(LR, 10), 2)
    assert bits_equal(pc, pa[:m].contiguous()) and bits_equal(sc, sa[:, :m].contiguous())


# ------------------------------------------------------------------------------------- the reference's fixtures ---
def _unplanes(planes, n):
    return np.ascontiguousarray(planes.transpose(0, 2, 1)).view(np.int32).reshape(planes.shape[0], n).astype(np.int64)


def _from_diffs(p0, d):
    return (p0.view(np.int32).astype(np.int64)[None] + np.cumsum(d, axis=0)).astype(np.int32).view(np.float32)


def recorded(z, name, n):
    """make_golden_optim.decode: the trajectories for the two weight decays, from the stored bit-pattern differences."""
    d0 = _unplanes(z[f"{name}.wd0"], n)
    return _from_diffs(z["p0"], d0), _from_diffs(z["p0"], d0 + _unplanes(z[f"{name}.wd1"], n))


def radam64(p0, grads, lr, wd, b1, b2, steps_per_grad, eps=1e-8):
    """Dassl/dassl/optim/radam.py:50-130 (degenerated_to_sgd=True) restated in float64; the parameters after every gradient."""
    p, m, v, t, out = p0.astype(np.float64).copy(), np.zeros(len(p0)), np.zeros(len(p0)), 0, []
    nmax = 2 / (1 - b2) - 1
    for g in grads.astype(np.float64):
        for _ in range(steps_per_grad):
            v = v * b2 + (1 - b2) * g * g
            m = m * b1 + (1 - b1) * g
            t += 1
            b2t = b2 ** t
            nsma = nmax - 2 * t * b2t / (1 - b2t)
            if wd != 0:
                p = p + (-wd * lr) * p
            if nsma >= 5:
                ss = np.sqrt((1 - b2t) * (nsma - 4) / (nmax - 4) * (nsma - 2) / nsma * nmax / (nmax - 2)) / (1 - b1 ** t)
                p = p + (-ss * lr) * m / (np.sqrt(v) + eps)
            else:
                p = p + (-lr / (1 - b1 ** t)) * m
        out.append(p.copy())
    return np.stack(out)


@pytest.mark.parametrize("wi", [0, 1], ids=["wd0", "wd5e-4"])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_trajectory_against_the_reference_fixture(kind, wi):
    meta = json.load(open(os.path.join(GOLD, "optim.json")))
    z = np.load(os.path.join(GOLD, "optim.npz"))
    n, reps, lr, wd, h = meta["n"], meta["steps_per_grad"], meta["lr"], meta["wds"][wi], meta["hyper"]
    assert meta["optims"] == ALL_KINDS and z["g"].shape == (8, 4096) and reps == 2
    assert np.all(z["g"][:, ::7] == 0.0) and np.count_nonzero(z["g"][:, 1::7]) == z["g"][:, 1::7].size
    rec = recorded(z, kind, n)[wi]
    spec = O.OptimSpec(kind=kind, beta1=h["beta1"], beta2=h["beta2"], alpha=h["alpha"], momentum=h["momentum"], weight_decay=wd)
    p0 = torch.from_numpy(z["p0"].copy())
    if kind == "radam":
        nsma = [v for _, v in meta["radam_nsma"]]
        assert len(nsma) == 16 and min(nsma) < 5 <= max(nsma)          # both branches inside the 16 steps
        ref64 = radam64(z["p0"], z["g"], lr, wd, h["beta1"], h["beta2"], reps)
    else:
        run = TorchRun(kind, p0, spec, lr, torch.float64)
        ref64 = np.stack([run.step(torch.from_numpy(gk.copy()), reps).p.numpy().copy() for gk in z["g"]])
    p, state = p0.cuda(), torch.zeros(spec.rows, n, device="cuda")
    msgs = []
    for k, gk in enumerate(z["g"]):
        ops.optim_step(p, torch.from_numpy(gk.copy()).cuda(), state, kind, spec.desc(lr, k * reps), reps)
        got = p.cpu().numpy().astype(np.float64)
        scale = np.abs(ref64[k] - z["p0"]).max()
        d_k, d_r = np.abs(got - ref64[k]).max() / scale, np.abs(rec[k].astype(np.float64) - ref64[k]).max() / scale
        msgs.append(f"grad {k}: kernel {d_k:.3e} recorded {d_r:.3e}")
        assert d_k <= 2 * d_r, f"{kind} wd={wd}: distance from float64 above 2 x the recorded float32 trajectory's: " + "; ".join(msgs)
    print(f"{kind} wd={wd}: " + "; ".join(msgs))


# -------------------------------------------------------------------------------------------------- bit identity ---
@pytest.mark.parametrize("n", [257, GRID_CAP + 4, VITB_N])
@pytest.mark.parametrize("kind", ALL_KINDS)
def test_entry_points_agree_bit_for_bit_and_the_device_counter_follows_the_host(kind, n):
    """After 1 call and after 5 consecutive calls with repeats = 2 (a new gradient each): eager, gated (good step) and _dev
    leave identical p and state rows; the device descriptor equals the host's (count and running powers) bit for bit."""
    spec = O.OptimSpec(kind=kind)
    p0, _, st = cpu_inputs(n, seed=11, rows=spec.rows, later=False)
    gs = [torch.randn(n, generator=torch.Generator().manual_seed(100 + i)).cuda() for i in range(5)]
    res = {}
    for entry in ("eager", "gated", "dev"):
        p, state = p0.cuda(), st.cuda().contiguous()
        sstate, desc = good_state(), None
        snap = []
        for i, g in enumerate(gs):
            lr = LR if i < 3 else LR / 4
            if entry == "dev" and desc is not None:
                desc[0:1].fill_(lr)
            desc = run_entry(entry, kind, p, g, state, spec, lr, 2 * i, 2, sstate if entry == "gated" else None, desc)
            if i in (0, 4):
                snap.append((p.clone(), state.clone()))
            if entry == "dev":
                torch.cuda.synchronize()
                assert bits_equal(desc.cpu(), torch.tensor(spec.desc_values(lr, 2 * (i + 1)), dtype=torch.float64)), (i, desc.tolist())
        res[entry] = snap
    for entry in ("gated", "dev"):
        for (pa, sa), (pb, sb), when in zip(res[entry], res["eager"], ("1 call", "5 calls")):
            assert bits_equal(pa, pb), f"{kind}: p of {entry} differs from eager after {when}"
            assert bits_equal(sa, sb), f"{kind}: state of {entry} differs from eager after {when}"
    assert not bits_equal(res["eager"][0][0], p0.cuda())


# --------------------------------------------------------------------------------------------------- fp16 gating ---
@pytest.mark.parametrize("kind", ["adamw", "amsgrad", "radam"])
def test_overflowed_step_moves_nothing_but_the_scale_and_the_next_step_is_t_plus_1(kind):
    spec = O.OptimSpec(kind=kind)
    n, t0 = GRID_CAP + 3, 6
    p0, g, st0 = cpu_inputs(n, seed=5, rows=spec.rows, later=True)
    p, state, g = p0.cuda(), st0.cuda().contiguous(), g.cuda()
    desc = dev_desc(spec, LR, t0)
    desc0 = desc.clone()
    ss = good_state(4096.0)
    ss[2] = 0.0
    ops.optim_step_dev(p, g, state, kind, desc, 2, ss)
    torch.cuda.synchronize()
    assert bits_equal(p, p0.cuda()) and bits_equal(state, st0.cuda()), "a skipped step moved the weights or a state row"
    assert bits_equal(desc, desc0), "a skipped step advanced the device count or the powers"
    assert float(ss[0]) == 2048.0 and float(ss[1]) == 1.0 / 2048.0 and float(ss[4]) == 1.0 and float(ss[3]) == 0.0
    # the host-descriptor entry point is gated the same way
    ph, sh = p0.cuda(), st0.cuda().contiguous()
    ss2 = good_state(4096.0)
    ss2[2] = 0.0
    ops.optim_step(ph, g, sh, kind, spec.desc(LR, t0), 2, ss2)
    torch.cuda.synchronize()
    assert bits_equal(ph, p0.cuda()) and bits_equal(sh, st0.cuda()) and float(ss2[0]) == 2048.0 and float(ss2[4]) == 1.0
    # the next good step applies step numbers t0+1, t0+2 - not t0+3, t0+4
    ss[2] = 1.0
    ops.optim_step_dev(p, g, state, kind, desc, 2, ss)
    pe, se = p0.cuda(), st0.cuda().contiguous()
    ops.optim_step(pe, g, se, kind, spec.desc(LR, t0), 2)
    pw, sw = p0.cuda(), st0.cuda().contiguous()
    ops.optim_step(pw, g, sw, kind, spec.desc(LR, t0 + 2), 2)
    torch.cuda.synchronize()
    assert bits_equal(p, pe) and bits_equal(state, se)
    assert not bits_equal(p, pw), "step numbers t0+3.. give the same bits: the check cannot tell them apart"
    assert bits_equal(desc.cpu(), torch.tensor(spec.desc_values(LR, t0 + 2), dtype=torch.float64))
    assert float(ss[3]) == 1.0 and float(ss[4]) == 1.0


@pytest.mark.parametrize("repeats", [0, 17])
def test_out_of_range_repeats_and_unknown_kind_run_nothing(repeats):
    spec = O.OptimSpec(kind="adam")
    p0, g, st0 = cpu_inputs(1000, seed=3, rows=2, later=True)
    p, state = p0.cuda(), st0.cuda().contiguous()
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.optim_step(p, g.cuda(), state, "adam", spec.desc(LR, 0), repeats)
    with pytest.raises(RuntimeError, match="invalid argument"):
        ops.optim_step_dev(p, g.cuda(), state, "adam", dev_desc(spec, LR, 0), repeats)
    with pytest.raises(ValueError):
        ops.optim_step(p, g.cuda(), state, "lion", spec.desc(LR, 0), 1)
    torch.cuda.synchronize()
    assert bits_equal(p, p0.cuda()) and bits_equal(state, st0.cuda())


# -------------------------------------------------------------------------------------------- engine integration ---
def to_dev(batch):
    return batch["img"].cuda(), batch["attrs"].t()[0].contiguous().cuda(), batch["label"].cuda()


@pytest.mark.parametrize("kind", ["adamw", "amsgrad"])
def test_engine_optim_step_against_torch_on_the_engines_own_gradients(kind):
    """Tiny ViT fp32, three steps of forward_backward + optim_step(repeats=2).  The matching torch.optim class is stepped
    twice per step on the CPU with the ENGINE's gradient buffer (not the oracle's gradients: Adam normalises the magnitude of a
    gradient away, so an element whose gradient sits at the level of the fp32 gradient error may move by a full lr in either
    direction - that would test gradient parity, which other tests hold)."""
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg, bs = C.vit_tiny(rank=4), 8
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.float32, max_images=bs)
    spec = O.OptimSpec(kind=kind, weight_decay=5e-4)
    p0 = eng.params.flat.cpu().clone()
    r32, r64 = TorchRun(kind, p0, spec, 2e-3, torch.float32), TorchRun(kind, p0, spec, 2e-3, torch.float64)
    for i in range(3):
        eng.forward_backward(*to_dev(synth.make_batch(mcfg, bs, seed=40 + i, signal=0.2)))
        g = eng.params.grad.cpu().clone()
        eng.optim_step(spec, 2e-3, repeats=2)
        r32.step(g, 2), r64.step(g, 2)
        assert eng.params.steps == 2 * (i + 1) and tuple(eng.params.optim_state.shape) == (spec.rows, eng.params.numel)
        assert eng.params.momentum.data_ptr() == eng.params.optim_state.data_ptr()
        # (parameters: the moments of real gradients are heavy-tailed, see cpu_inputs; they are printed, not bounded)
        check_bound(f"engine {kind} step {i}", eng.params.flat.cpu(), list(eng.params.optim_state.cpu()), p0, r32, r64, rows=False)
    assert float(g.abs().max()) > 0


def test_engine_fp16_overflowed_optim_step_is_skipped_and_the_count_stays():
    """fp16 engine at grad_scale 2^30: every overflowed step leaves weights and state rows bitwise alone, optim_steps() (the
    device counter) does not move and the scale halves; good steps then advance it by `repeats`.  params.steps counts the
    applications ATTEMPTED and is only an upper bound here."""
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg, bs = C.vit_tiny(rank=4), 8
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    eng = FairLoRAEngine(mcfg, sd, dtype=torch.float16, max_images=bs)
    eng.grad_scale = 2.0 ** 30
    spec = O.OptimSpec(kind="adamw")
    batch = to_dev(synth.make_batch(mcfg, bs, seed=1234))
    skipped = good = 0
    for i in range(40):
        flat, state, count, scale = eng.params.flat.clone(), None if i == 0 else eng.params.optim_state.clone(), eng.optim_steps(), eng.grad_scale
        eng.forward_backward(*batch)
        eng.optim_step(spec, 2e-3, repeats=2)
        torch.cuda.synchronize()
        if float(eng.scale_state[2]) == 0.0:
            skipped += 1
            assert bits_equal(eng.params.flat, flat) and (state is None or bits_equal(eng.params.optim_state, state))
            assert eng.optim_steps() == count and eng.grad_scale == scale / 2 and eng.overflow_steps() == skipped
        else:
            good += 1
            assert not bits_equal(eng.params.flat, flat) and eng.optim_steps() == count + 2
            if good == 2:
                break
    assert skipped > 0 and good == 2 and eng.optim_steps() == 4 and eng.params.steps == 2 * (skipped + good)
    assert bool(torch.isfinite(eng.params.flat).all())


def make_cfg(optim, prec="fp32", bs=8):
    return NS(
        SEED=1, OUTPUT_DIR="", VERBOSE=False,
        INPUT=NS(PIXEL_MEAN=list(C.CLIP_PIXEL_MEAN), PIXEL_STD=list(C.CLIP_PIXEL_STD), SIZE=(64, 64)),
        DATASET=NS(NAME="FairFedMed", ATTRIBUTES=["race"], ATTRIBUTE_TYPE="race"),
        MODEL=NS(BACKBONE=NS(NAME="tiny"), GEOMETRY=C.vit_tiny(), STATE_DICT=None),
        TRAINER=NS(NAME="GLP_OT_SVLoRA", LAMBDA_FAIRNESS=0.0,
                   GLP_OT=NS(N=2, N_CTX=4, PREC=prec, OT="None"),
                   GLP_OT_LORA=NS(RANK=4, ALPHA=2.0, TYPE="FairLoRA", GLOBAL_S=False, DISABLE_ATTR=False,
                                  UNFREEZE_IMAGE_ENCODER=True)),
        OPTIM=optim,
        DATALOADER=NS(TRAIN_X=NS(BATCH_SIZE=bs)), TEST=NS(BATCH_SIZE=bs, NO_TEST=True),
        TRAIN=NS(METRICS_EVERY=1, CHECKPOINT_FREQ=0),
    )


def make_trainer(optim, sd, prec="fp32"):
    from fairfedmed_amd.trainer import GLP_OT_SVLoRA, SyntheticFedData
    mcfg = C.vit_tiny(rank=4)
    data = SyntheticFedData(mcfg, num_clients=1, train_batches=3, test_batches=1, batch_size=8, signal=0.3)
    return GLP_OT_SVLoRA(make_cfg(optim, prec), data=data, state_dict=sd)


def spy_on_steps(tr):
    """Record (entry, lr, gradient on the CPU) of every optimizer call the trainer makes."""
    calls = []
    eng = tr.engine
    sgd, opt = eng.sgd_step, eng.optim_step

    def sgd_step(lr, *a, **k):
        calls.append(("sgd_step", lr, None))
        return sgd(lr, *a, **k)

    def optim_step(spec, lr, repeats=1):
        calls.append(("optim_step", lr, eng.params.grad.cpu().clone()))
        assert repeats == 2
        return opt(spec, lr, repeats=repeats)

    eng.sgd_step, eng.optim_step = sgd_step, optim_step
    return calls


def adamw_cosine_cfg():
    """OPTIM of fixture 'cosine|constant2|5': AdamW, cosine over MAX_EPOCH = 5, two epochs of constant warm-up."""
    return NS(NAME="adamw", LR=2e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, LR_SCHEDULER="cosine", STEPSIZE=(-1,), GAMMA=0.1, MAX_EPOCH=5,
              WARMUP_EPOCH=2, WARMUP_TYPE="constant", WARMUP_CONS_LR=1e-5, WARMUP_MIN_LR=1e-5, WARMUP_RECOUNT=True)


def test_trainer_adamw_cosine_warmup_lrs_parameters_and_round_trips(tmp_path):
    meta = json.load(open(os.path.join(GOLD, "optim.json")))
    rec = meta["sched"]["cosine|constant2|5"]
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    tr = make_trainer(adamw_cosine_cfg(), sd)
    assert tr.optim_spec.kind == "adamw" and tr.sched.name == "cosine" and tr.steps_per_update() == 2
    assert tuple(tr.engine.params.optim_state.shape) == (2, tr.engine.params.numel)
    p0 = tr.engine.params.flat.cpu().clone()
    calls = spy_on_steps(tr)
    for _ in range(2):                               # two local epochs of three batches
        tr.run_epoch(0)
    assert [c[0] for c in calls] == ["optim_step"] * 6
    # the scheduler is stepped twice per epoch (once per registered name): epoch e sees the LR after 2e step() calls
    want = [rec["lr0"]] * 3 + [rec["lrs"][1]] * 3
    for (_, lr, _), w in zip(calls, want):
        assert lr == w or abs(lr - w) <= 1e-12 * abs(w), ([c[1] for c in calls], want)
    assert abs(tr.get_current_lr() - rec["lrs"][3]) <= 1e-12 * rec["lrs"][3] and tr.sched.last_epoch == 4
    # parameters: torch.optim.AdamW stepped twice per batch with the engine's own gradients and the same LRs
    r32, r64 = (TorchRun("adamw", p0, tr.optim_spec, 2e-3, dt) for dt in (torch.float32, torch.float64))
    for _, lr, g in calls:
        r32.step(g, 2, lr=lr), r64.step(g, 2, lr=lr)
    check_bound("trainer adamw", tr.engine.params.flat.cpu(), list(tr.engine.params.optim_state.cpu()), p0, r32, r64, rows=False)
    # optimizer_state() / load_optimizer_state(): a second trainer picks the state up and trains on bit-identically
    mom, scal = tr.optimizer_state()
    assert mom.numel() == 2 * tr.engine.params.numel and scal.tolist() == [12.0, 4.0, tr.get_current_lr()]
    weights = {k: v.clone() for k, v in tr.model.state_dict().items()}
    tr.save_model(0, str(tmp_path), is_best=True)
    other = make_trainer(adamw_cosine_cfg(), sd)
    other.model.load_state_dict(weights, strict=False)
    other.load_optimizer_state(mom.clone(), scal.clone())
    third = make_trainer(adamw_cosine_cfg(), sd)
    third.load_model(str(tmp_path))
    for t in (tr, other, third):
        t.run_epoch(0)
    for name, t in (("load_optimizer_state", other), ("load_model", third)):
        assert bits_equal(t.engine.params.flat, tr.engine.params.flat), f"{name}: weights differ after a further epoch"
        assert bits_equal(t.engine.params.optim_state, tr.engine.params.optim_state), f"{name}: optimizer state differs"
        assert t.get_current_lr() == tr.get_current_lr() and t.sched.last_epoch == 6 and t.engine.params.steps == 18
    assert not bits_equal(tr.engine.params.flat.cpu(), p0)


# -------------------------------------------------------------------------------------------------- captured step ---
def opt_state_of(eng):
    p = eng.params
    out = {"flat": p.flat.clone(), "optim_state": p.optim_state.clone(), "steps": p.steps}
    if eng.scale_state is not None:
        out["scale_state"] = eng.scale_state.clone()
    if p.optim_desc is not None:
        out["desc"] = p.optim_desc.clone()
    return out


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
def test_captured_adamw_step_is_bit_identical_to_three_eager_steps(dtype):
    from fairfedmed_amd.engine import FairLoRAEngine
    mcfg, bs = C.vit_tiny(rank=4), 8
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    batches = [to_dev(synth.make_batch(mcfg, bs, seed=40 + i, signal=0.2)) for i in range(3)]
    eager, graphed = (FairLoRAEngine(mcfg, sd, dtype=dtype, max_images=bs) for _ in range(2))
    spec = O.OptimSpec(kind="adamw", weight_decay=5e-4)
    before = graphed.params.flat.clone()
    step = graphed.capture_train_step(bs, 2e-3, spec.momentum, spec.weight_decay, repeats=2, optimizer=spec)
    torch.cuda.synchronize()
    assert bits_equal(graphed.params.flat, before) and graphed.params.steps == 0          # capturing leaves no trace
    assert float(graphed.params.optim_state.abs().max()) == 0.0 and float(graphed.params.optim_desc[9]) == 0.0
    lr = 2e-3
    for i, (img, attr, label) in enumerate(batches):
        if i == 1:                                    # the LR schedule moves between replays
            lr = 5e-4
            step.set_lr(lr)
        loss_e = eager.forward_backward(img, attr, label)["loss"].clone()
        eager.optim_step(spec, lr, repeats=2)
        loss_g = step.run(img, attr, label)["loss"].clone()
        torch.cuda.synchronize()
        assert bits_equal(loss_g, loss_e)
        a, b = opt_state_of(graphed), opt_state_of(eager)
        for k in ("flat", "optim_state") + (("scale_state", "desc") if dtype == torch.float16 else ()):
            assert bits_equal(a[k], b[k]), f"step {i}: {k} of the graphed engine differs from the eager one"
        assert a["steps"] == b["steps"] == 2 * (i + 1)
        assert bits_equal(a["desc"].cpu(), torch.tensor(spec.desc_values(lr, 2 * (i + 1)), dtype=torch.float64))
        assert bool(torch.isfinite(a["flat"]).all()) and not bits_equal(a["flat"], before)


# ------------------------------------------------------------------------------------------- unchanged behaviour ---
def test_config_without_the_new_keys_is_the_sgd_path_bit_for_bit():
    """No NAME / LR_SCHEDULER / WARMUP_*: sgd_step, one state row, StepLR - and two trainers built from the same config and
    state dict train bit-identically (the new paths add no state and no reordering)."""
    old = lambda: NS(LR=1e-3, MOMENTUM=0.9, WEIGHT_DECAY=5e-4, STEPSIZE=2, GAMMA=0.1, MAX_EPOCH=1)     # noqa: E731
    mcfg = C.vit_tiny(rank=4)
    sd = synth.make_state_dict(mcfg, seed=1, lora_init="random")
    a, b = make_trainer(old(), sd), make_trainer(old(), sd)
    calls = spy_on_steps(a)
    for t in (a, b):
        assert t.optim_spec.kind == "sgd" and t.sched.name == "single_step" and t.sched.warmup_epoch <= 0
        assert tuple(t.engine.params.optim_state.shape) == (1, t.engine.params.numel) and t.engine.params.optim_desc is None
        t.num_batches = 10 ** 9
        batch = synth.make_batch(mcfg, 8, seed=1234)
        for i in range(2):
            t.batch_idx = i
            t.forward_backward(batch)
    assert [c[0] for c in calls] == ["sgd_step", "sgd_step"] and [c[1] for c in calls] == [1e-3, 1e-3]
    assert bits_equal(a.engine.params.flat, b.engine.params.flat) and bits_equal(a.engine.params.momentum, b.engine.params.momentum)
    mom, scal = a.optimizer_state()
    assert mom.data_ptr() == a.engine.params.momentum.data_ptr() and tuple(mom.shape) == (a.engine.params.numel,)
    assert scal.tolist() == [4.0, 0.0, 1e-3]
    a.update_lr()
    assert a.sched.last_epoch == 2 and a.get_current_lr() == 1e-3 * 0.1 ** 1
