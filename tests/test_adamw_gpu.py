"""The fused AdamW on the GPU: klab_adamw_step_range through the C ABI against the fp64 reference of tests/adamw_ref.py (per-element
bounds proved in tests/test_adamw_cpu.py; tables in LDS, n = 5, and in global memory, n = 1100; 1, 3 and 16 parameter groups), and
optim.FusedAdamW on the tiny golden models against torch.optim.AdamW: two groups, a scheduler per group, step_in_backward, klab DDP
with overlap_optimizer, clipping first, resume and re-bind."""
import os
import types

import pytest
import torch

from tests import adamw_ref as A
from tests.adamw_ref import bits
from tests.helpers import load_golden, rel_l2

pytestmark = pytest.mark.gpu

NTAB = (5, 1100)  # 1100 > 1024: the descriptor and group tables are read from global memory


@pytest.fixture(scope="module")
def ops():
    from klab_multimodalmodel_amd import ops as K
    return K


@pytest.fixture(scope="module")
def states():
    return {n: A.AdamWState(n, seed=63) for n in NTAB}


def launch(ops, s, groups, gof, begin4=0, end4=None, arena=None):
    """one klab_adamw_step_range over the state's buffers -> (p, m, v, arena) on the host; g must come back untouched"""
    arena = s.arena if arena is None else arena
    pd, gd, md, vd, ad = s.p.cuda(), s.g.cuda(), s.m.cuda(), s.v.cuda(), arena.cuda()
    desc = torch.tensor([[pd.data_ptr() + 4 * po, go, ao, p4] for po, go, ao, p4 in zip(s.poff, s.goff, s.aoff, s.pre)], dtype=torch.int64).cuda()
    gid = torch.tensor(gof, dtype=torch.int32).cuda()
    try:
        ops.adamw_step(desc, gid, groups, gd, md, vd, ad, begin4=begin4, end4=end4, total4=s.total4)
    finally:
        torch.cuda.synchronize()
        out = pd.cpu(), md.cpu(), vd.cpu(), ad.cpu()
        assert torch.equal(bits(gd.cpu()), bits(s.g))
    return out


def check_outside(s, out, arena=None):
    """nothing outside the tensors, nothing in the arena for tensors without a copy: bit for bit"""
    arena = s.arena if arena is None else arena
    p1, m1, v1, a1 = out
    mp, mg, ma = s.masks(range(s.n))
    assert torch.equal(bits(p1)[~mp], bits(s.p)[~mp]) and torch.equal(bits(m1)[~mg], bits(s.m)[~mg]) and torch.equal(bits(v1)[~mg], bits(s.v)[~mg])
    assert torch.equal(bits(a1)[~ma], bits(arena)[~ma])


def check_groups(s, out, groups, gof, label):
    """every tensor against the reference of ITS group"""
    p1, m1, v1, a1 = out
    for k, h in enumerate(groups):
        idx = [i for i in range(s.n) if gof[i] == k]
        assert idx
        P, P1 = s.gather(s.p, s.poff, idx), s.gather(p1, s.poff, idx)
        G, M, V = (s.gather(t, s.goff, idx) for t in (s.g, s.m, s.v))
        M1, V1 = s.gather(m1, s.goff, idx), s.gather(v1, s.goff, idx)
        rm, rv, rp = A.errors(P, P1, M1, V1, A.adamw_ref(P, G, M, V, h))
        print(f"adamw {label} group {k}: m {rm:.2f} ulp, v {rv:.2f} ulp, dp err / bound {rp:.3f}")
        assert rm <= A.M_V_ULPS and rv <= A.M_V_ULPS, (label, k, rm, rv)
        assert rp <= 1.0, (label, k, rp)
        assert not torch.equal(M1, M) and not torch.equal(V1, V)
        if h["lr"] == 0.0:
            assert torch.equal(bits(P1), bits(P))  # lr = 0: the parameter keeps its bits ...
        else:
            assert not torch.equal(bits(P1), bits(P))
        with_a = [i for i in idx if s.has_a[i]]
        if with_a:  # ... and the arena copy is (re)written from it
            want = s.gather(p1, s.poff, with_a).to(a1.dtype)
            assert torch.equal(bits(s.gather(a1, s.aoff, with_a)), bits(want))


# ---- the kernel through the C ABI -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("n", NTAB)
def test_single_group_matches_fp64_adamw(ops, states, n, wd):
    s = states[n]
    groups, gof = A.one_group(wd), [0] * n
    out = launch(ops, s, groups, gof)
    check_outside(s, out)
    check_groups(s, out, groups, gof, f"n={n} wd={wd}")
    P, P1 = s.gather(s.p, s.poff), s.gather(out[0], s.poff)
    assert float((P1.double() - P.double()).abs().min()) > 0  # every element moved


@pytest.mark.parametrize("n", NTAB)
def test_three_groups_each_tensor_follows_its_own_group(ops, states, n):
    s = states[n]
    groups, gof = A.three_groups(), s.groups_of(3)
    assert groups[A.ZERO_LR_GROUP]["lr"] == 0.0
    out = launch(ops, s, groups, gof)
    check_outside(s, out)
    check_groups(s, out, groups, gof, f"n={n} 3 groups")
    # the references of two groups are far apart: a tensor updated with a neighbour's hyper-parameters could not pass
    i = next(i for i in range(n) if gof[i] == 0)
    P, G, M, V = s.p[s.poff[i]:][:s.lens[i]], s.g[s.goff[i]:][:s.lens[i]], s.m[s.goff[i]:][:s.lens[i]], s.v[s.goff[i]:][:s.lens[i]]
    d0, d1 = A.adamw_ref(P, G, M, V, groups[0])[2], A.adamw_ref(P, G, M, V, groups[1])[2]
    assert float((d0 - d1).abs().min()) > 100 * 3 * A.U24 * 2


def test_sixteen_groups(ops, states):
    s = states[1100]
    groups, gof = A.sixteen_groups(), s.groups_of(16)
    out = launch(ops, s, groups, gof)
    check_outside(s, out)
    check_groups(s, out, groups, gof, "n=1100 16 groups")


def test_seventeen_groups_are_refused_and_nothing_runs(ops, states):
    from klab_multimodalmodel_amd import _lib
    s = states[5]
    groups = A.sixteen_groups() + [A.group(1e-3, 0.9, 0.999, 1e-8, 0.0)]
    with pytest.raises(NotImplementedError):
        launch(ops, s, groups, s.groups_of(17))
    # the raw return value, and the buffers bit for bit
    pd, gd, md, vd, ad = s.p.cuda(), s.g.cuda(), s.m.cuda(), s.v.cuda(), s.arena.cuda()
    desc = torch.tensor([[pd.data_ptr() + 4 * po, go, ao, p4] for po, go, ao, p4 in zip(s.poff, s.goff, s.aoff, s.pre)], dtype=torch.int64).cuda()
    gid = torch.tensor(s.groups_of(17), dtype=torch.int32).cuda()
    rc = _lib.load().klab_adamw_step_range(desc.data_ptr(), s.n, gid.data_ptr(), _lib.adamw_groups(groups), 17, 0, s.total4, gd.data_ptr(),
                                           md.data_ptr(), vd.data_ptr(), ad.data_ptr(), _lib.BF16, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED
    for got, before in ((pd, s.p), (gd, s.g), (md, s.m), (vd, s.v), (ad, s.arena)):
        assert torch.equal(bits(got.cpu()), bits(before))


@pytest.mark.parametrize("n", NTAB)
def test_sub_range_touches_only_its_tensors(ops, states, n):
    s = states[n]
    groups, gof = A.three_groups(), s.groups_of(3)
    full = launch(ops, s, groups, gof)
    i0, i1 = (1, 4) if n == 5 else (n // 3, 2 * n // 3)
    part = launch(ops, s, groups, gof, begin4=s.pre[i0], end4=s.pre[i1])
    mp, mg, ma = s.masks(range(i0, i1))
    for got, whole, before, inside in zip(part, full, (s.p, s.m, s.v, s.arena), (mp, mg, mg, ma)):
        assert torch.equal(bits(got)[inside], bits(whole)[inside])     # the same update inside the range
        assert torch.equal(bits(got)[~inside], bits(before)[~inside])  # bit for bit untouched outside it
    assert not torch.equal(part[1][mg], s.m[mg])


@pytest.mark.parametrize("n", NTAB)
def test_fp32_arena_holds_the_parameter_exactly(ops, states, n):
    s = states[n]
    arena = torch.full((len(s.arena),), float("nan"), dtype=torch.float32)
    groups, gof = A.three_groups(), s.groups_of(3)
    out = launch(ops, s, groups, gof, arena=arena)
    check_outside(s, out, arena)
    with_a = [i for i in range(n) if s.has_a[i]]
    assert out[3].dtype == torch.float32
    assert torch.equal(bits(s.gather(out[3], s.aoff, with_a)), bits(s.gather(out[0], s.poff, with_a)))
    bf = launch(ops, s, groups, gof)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(out[:3], bf[:3]))  # the arena's type changes nothing else


# ---- optim.FusedAdamW on the tiny models ----------------------------------------------------------------------------------------------
def build(name="tiny_a", dtype=torch.float32, train_swin=False, train=False):
    from klab_multimodalmodel_amd.engine import SwinConfig, T5Config
    from klab_multimodalmodel_amd.models.model import MyModel
    g = load_golden(name)
    sw, t5 = SwinConfig.from_dict(g["meta"]["swin_config"]), T5Config.from_dict(g["meta"]["t5_config"])
    args = types.SimpleNamespace(result_dir="/tmp", language_model_name="-", image_model_name="-", image_model_train=train_swin,
                                 transformer_model_name="-")
    m = MyModel(args, _configs=(sw, t5, t5), _state_dicts=(g["sds"]["swin"], g["sds"]["lang"], g["sds"]["main"]), dtype=dtype).to("cuda")
    m._direct_grads = True
    m.transformer.train(train)
    return m, g


def run(m, g, rows=None, lt=None):
    """the golden batch, or its first `rows` rows with the targets cut to `lt` tokens (another binding of the engine)"""
    inp = g["inputs"]
    pix, src, tgt = inp["pixel_values"][:rows], inp["src_ids"][:rows], inp["tgt_ids"][:rows, :lt]
    return m({"pixel_values": pix.cuda()}, {"input_ids": src.cuda()}, {"input_ids": tgt.contiguous().cuda()})


def two_groups(m):
    """decay 0.1 on the matrices; the norm weights and the position bias undecayed, with hyper-parameters of their own"""
    from klab_multimodalmodel_amd.optim import decay_param_groups
    core = m.module if hasattr(m, "module") else m
    gs = decay_param_groups(core, 0.1)
    gs[1].update(lr=1e-3, betas=(0.8, 0.99), eps=1e-6)
    return gs


def train(m, g, opt, n, sched=None, clip=None, **kw):
    out = []
    for _ in range(n):
        loss = run(m, g, **kw)
        loss.backward()
        if clip is not None:
            clip(opt)
        opt.step()
        opt.zero_grad()
        if sched is not None:
            sched.step()
        out.append(float(loss))
    return out


def worst_param(ma, mb):
    return max(rel_l2(b.detach().cpu(), a.detach().cpu()) for (_n, a), (_k, b) in zip(ma.transformer.named_parameters(), mb.transformer.named_parameters()))


def assert_follows_torch(dtype, make_sched=None, clip=None, steps=4, groups=None):
    """torch.optim.AdamW and optim.FusedAdamW on the same two groups, `steps` steps in eval mode: the tolerances of
    test_fused_adam_matches_torch_adam"""
    from klab_multimodalmodel_amd.optim import FusedAdamW
    ms, opts, losses = [], [], []
    for fused in (False, True):
        m, g = build("tiny_a", dtype)
        opt = (FusedAdamW if fused else torch.optim.AdamW)((groups or two_groups)(m), lr=3e-3)
        losses.append(train(m, g, opt, steps, make_sched(opt) if make_sched else None, clip))
        ms.append(m)
        opts.append(opt)
    f32 = dtype == torch.float32
    assert opts[1]._fallback is None and opts[1]._fb_reason is None, opts[1]._fb_reason  # the one-launch path really ran
    assert ms[1]._trainable_current()                                                      # ... and the next forward skips its cast
    for a, b in zip(*losses):
        assert abs(a - b) <= (2e-5 if f32 else 2e-3) * abs(a) + 1e-6, losses
    worst = worst_param(ms[0], ms[1])
    assert worst < (1e-5 if f32 else 2e-2), worst
    assert losses[0][0] != losses[0][-1]
    return ms, opts


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_two_groups_follow_torch_adamw(dtype):
    ms, opts = assert_follows_torch(dtype)
    f32 = dtype == torch.float32
    # both groups have tensors in both backward segments: the segment-wise tests below exercise every group twice
    ptrs, n0 = ms[1]._engine.adam_layout()
    gof = {p.data_ptr(): k for k, grp in enumerate(opts[1].param_groups) for p in grp["params"]}
    assert 0 < n0 < len(ptrs) == len(gof)
    for k in (0, 1):
        assert any(gof[q] == k for q in ptrs[:n0]) and any(gof[q] == k for q in ptrs[n0:])
    assert opts[1]._gid.cpu().tolist() == [gof[q] for q in ptrs]
    # torch.optim.AdamW's state dict: the groups, and the moments of one parameter of each group
    sd, ref = opts[1].state_dict(), opts[0].state_dict()
    assert set(sd["state"]) == set(ref["state"]) and [g["params"] for g in sd["param_groups"]] == [g["params"] for g in ref["param_groups"]]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.1, 0.0] and sd["param_groups"][1]["betas"] == (0.8, 0.99)
    for grp in sd["param_groups"]:
        k = grp["params"][0]
        assert set(sd["state"][k]) >= {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][k]["step"]) == 4.0
        assert rel_l2(sd["state"][k]["exp_avg"].cpu(), ref["state"][k]["exp_avg"].cpu()) < (1e-4 if f32 else 2e-2)
    # a state saved by the fused class continues in torch's
    fresh = torch.optim.AdamW(two_groups(ms[0]), lr=1.0)
    fresh.load_state_dict(sd)
    assert fresh.param_groups[1]["lr"] == 1e-3 and float(fresh.state[fresh.param_groups[1]["params"][0]]["step"]) == 4.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_a_scheduler_per_group(dtype):
    make = lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 1.0 / (1 + e), lambda e: 0.5 ** e])
    _ms, opts = assert_follows_torch(dtype, make_sched=make)
    assert [g["lr"] for g in opts[1].param_groups] == [g["lr"] for g in opts[0].param_groups]
    assert [g["lr"] for g in opts[1].param_groups] == pytest.approx([3e-3 / 5, 1e-3 / 16], rel=1e-12)


def exact_beta_groups(m):
    """two_groups with betas that f32 holds exactly, 1 - beta included (those of the kernel tests)"""
    gs = two_groups(m)
    gs[0].update(betas=(0.875, 1 - 2.0 ** -10))
    gs[1].update(betas=(0.75, 1 - 2.0 ** -7))
    return gs


def test_clipping_first_keeps_the_fused_path():
    """optim.clip_grad_norm_(..., 0.5) then FusedAdamW.step() against torch's clip and torch.optim.AdamW, the tolerances of the
    parity test.  The betas are ones that f32 holds exactly.  The C ABI carries the hyper-parameters as f32, and f32(0.999) is
    1.3e-8 above 0.999: 1 - beta2, and with it v, is 1.3e-5 smaller than torch's, every update 6e-6 larger.  Without clipping that
    offset stays what it is (2.6e-6 of the parameters after 4 steps, measured; the parity test's bound has room for it).  Clipped
    to 0.5 the gradients reach the optimizer scaled by 0.09, 0.20, 0.28, 0.29 in the four steps (total norms 5.5, 2.5, 1.8, 1.7), so
    each new gradient outweighs the second moment it meets, the steps are up to three times lr, and the trajectory carries a
    perturbation of the updates forward with a gain of ~160: default betas end 4.2e-4 apart (measured, rel-L2 of
    encoder.block.1.layer.1.DenseReluDense.wi.weight), torch against torch on two runs 1.9e-7.  What this test is about -- the
    clipped gradients stay where the fused step reads them, and both fused paths are kept -- does not depend on how 0.999 rounds,
    so the rounding is taken out of the comparison and the tolerance is kept."""
    from klab_multimodalmodel_amd import optim

    def clip(opt):
        ps = [p for g in opt.param_groups for p in g["params"]]
        if isinstance(opt, optim.FusedAdamW):
            total = optim.clip_grad_norm_(ps, 0.5)
            assert total.is_cuda and float(total) > 0.5  # really clipped
        else:
            torch.nn.utils.clip_grad_norm_(ps, 0.5)
    assert_follows_torch(torch.float32, clip=clip, groups=exact_beta_groups)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_step_in_backward_matches_the_ordinary_step(dtype):
    """the assertions of test_fused_adam_step_in_backward, with two groups: 5 steps, dropout on"""
    from klab_multimodalmodel_amd.optim import FusedAdamW
    ms, opts = [], []
    for inb in (False, True):
        m, g = build("tiny_b", dtype, train=True)
        opts.append(FusedAdamW(two_groups(m), lr=2e-3, step_in_backward=inb))
        ms.append(m)
    for step in range(5):
        ls = [train(ms[k], g, opts[k], 1)[0] for k in (0, 1)]
        assert abs(ls[0] - ls[1]) <= (2e-5 if dtype == torch.float32 else 3e-3) * abs(ls[0]) + 1e-6, (step, ls)
    assert opts[1]._fallback is None and opts[1].in_backward_updates == 4 and opts[0].in_backward_updates == 0
    assert ms[1]._trainable_current()
    assert worst_param(ms[0], ms[1]) < (1e-5 if dtype == torch.float32 else 2e-2)
    assert rel_l2(opts[1]._m.cpu(), opts[0]._m.cpu()) < (1e-4 if dtype == torch.float32 else 3e-2)
    assert rel_l2(opts[1]._v.cpu(), opts[0]._v.cpu()) < (1e-4 if dtype == torch.float32 else 3e-2)
    # a backward whose step() never comes: the next forward still orders itself behind the in-flight segment-0 update
    run(ms[1], g).backward()
    assert ms[1]._pending_opt_stream is not None
    with torch.no_grad():
        run(ms[1], g)
    assert ms[1]._pending_opt_stream is None
    torch.cuda.synchronize()


@pytest.mark.parametrize("cls", ["FusedAdamW", "FusedAdam"])
def test_a_second_backward_before_step_is_refused(cls):
    """gradient accumulation under step_in_backward=True: segment 0 was already updated underneath the first backward, and the
    second one finds every .grad set (no "fresh" segment that would ask the optimizer)"""
    from klab_multimodalmodel_amd import optim
    m, g = build("tiny_a")
    opt = getattr(optim, cls)(two_groups(m) if cls == "FusedAdamW" else m.transformer.parameters(), lr=1e-3, step_in_backward=True)
    train(m, g, opt, 1)  # the first step runs the ordinary way and registers the optimizer with the model
    assert opt._fallback is None and opt.in_backward_updates == 0
    run(m, g).backward()
    assert opt.in_backward_updates == 1 and opt._bw_token is not None
    loss = run(m, g)
    with pytest.raises(RuntimeError, match=rf"{cls}\(step_in_backward=True\) supports exactly one backward\(\) per step\(\)"):
        loss.backward()
    assert opt.in_backward_updates == 1
    with torch.no_grad():
        assert torch.isfinite(run(m, g))  # a forward afterwards still works
    torch.cuda.synchronize()


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_klab_ddp_overlap_optimizer_matches_no_wrapper():
    """one NCCL rank (the recipe of test_reference_training_loop_under_stock_ddp_and_klab_ddp): segment 0 is updated while segment 1
    is still being reduced"""
    import gc
    import torch.distributed as dist
    from klab_multimodalmodel_amd.ddp import DistributedDataParallel
    from klab_multimodalmodel_amd.optim import FusedAdamW

    def steps(wrap):
        m, g = build("tiny_b", torch.float32, train_swin=True)
        model = DistributedDataParallel(m, device_ids=[0], overlap_optimizer=True) if wrap else m
        opt = FusedAdamW(two_groups(m), lr=1e-3)
        losses = train(model, g, opt, 3)
        assert opt._fallback is None, opt._fb_reason
        w = {k: v.detach().clone() for k, v in m.transformer.state_dict().items()}
        torch.cuda.synchronize()
        return losses, w

    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
    try:
        l0, w0 = steps(False)
        os.environ["KLAB_DDP_FORCE_COLLECTIVE"] = "1"  # the all-reduces are really issued on the communication stream
        try:
            l1, w1 = steps(True)
        finally:
            del os.environ["KLAB_DDP_FORCE_COLLECTIVE"]
        assert max(abs(x - y) for x, y in zip(l0, l1)) < 2e-4, (l0, l1)
        for k in w0:
            assert rel_l2(w1[k].cpu(), w0[k].cpu()) < 2e-3, k
        assert l0[0] > l0[-1]
    finally:
        gc.collect()  # klab DDP-wrapped models sit in a reference cycle with their wrapper
        torch.cuda.synchronize()
        dist.destroy_process_group()


@pytest.mark.parametrize("how", ["checkpointer", "state_dict"])
def test_resume_continues_four_uninterrupted_steps(tmp_path, how):
    from klab_multimodalmodel_amd.checkpoint import AsyncCheckpointer, load_checkpoint
    from klab_multimodalmodel_amd.optim import FusedAdamW

    def make(lr=2e-3):
        m, g = build("tiny_a")
        m.args.result_dir = str(tmp_path)
        return m, g, FusedAdamW(two_groups(m), lr=lr)

    m0, g, o0 = make()
    ref = train(m0, g, o0, 4)
    m1, g, o1 = make()
    first = train(m1, g, o1, 2)
    m2, g, o2 = make(lr=7.0)  # (the saved groups bring their learning rates back)
    if how == "checkpointer":
        ck = AsyncCheckpointer(str(tmp_path))
        path = ck.save(m1, o1, None, step=2, name="s.pth")
        ck.wait()
        assert os.path.exists(path + ".opt0of1")  # the flat state, not a state dict
        with torch.no_grad():
            run(m2, g)  # binds the engine: the flat buffers exist
        assert load_checkpoint(path, m2, o2) == 2
    else:
        m1.save("ck.pth")
        torch.save(o1.state_dict(), os.path.join(str(tmp_path), "opt.pth"))
        m2.load("ck.pth")
        with torch.no_grad():
            run(m2, g)
        o2.load_state_dict(torch.load(os.path.join(str(tmp_path), "opt.pth")))
    assert [(grp["lr"], grp["weight_decay"], tuple(grp["betas"]), grp["eps"]) for grp in o2.param_groups] == \
        [(2e-3, 0.1, (0.9, 0.999), 1e-8), (1e-3, 0.0, (0.8, 0.99), 1e-6)]
    rest = train(m2, g, o2, 2)
    assert o2._fallback is None and o2._steps == 4, o2._fb_reason
    for a, b in zip(ref, first + rest):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, (ref, first + rest)


def test_a_rebind_between_steps_keeps_the_fused_path():
    """the reference loop pads every batch to its longest row, so (B, Ls, Lt) changes almost every step: the group table is the
    optimizer's and survives"""
    from klab_multimodalmodel_amd.optim import FusedAdamW
    ms, opts, losses = [], [], []
    for fused in (False, True):
        m, g = build("tiny_a")
        opt = (FusedAdamW if fused else torch.optim.AdamW)(two_groups(m), lr=3e-3)
        ls = train(m, g, opt, 1)
        table = opt._gid if fused else None
        ls += train(m, g, opt, 1, rows=2, lt=5)  # another (B, Lt): a re-bind
        ls += train(m, g, opt, 1)                # and back
        if fused:
            assert opt._fallback is None and opt._gid is table and opt._steps == 3, opt._fb_reason
            assert m._trainable_current()
        ms.append(m)
        losses.append(ls)
    for a, b in zip(*losses):
        assert abs(a - b) <= 2e-5 * abs(a) + 1e-6, losses
    assert worst_param(ms[0], ms[1]) < 1e-5


def test_seventeen_param_groups_step_in_torch():
    from klab_multimodalmodel_amd.optim import FusedAdamW
    m, g = build("tiny_a")
    ps = [p for p in m.transformer.parameters()]
    assert len(ps) >= 17
    groups = [{"params": [p]} for p in ps[:16]] + [{"params": ps[16:]}]
    opt = FusedAdamW(groups, lr=1e-3)
    train(m, g, opt, 1)
    assert opt._fallback is not None and opt._fb_reason == "more than 16 param groups"
