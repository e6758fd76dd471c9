"""GPU: the fused optimiser step (ntm_amd.optim.FusedAdam, ema_update_; csrc/multi_tensor.hip) at the smallest shapes at which the
kernels can go wrong -- chunk and table edges, the scalar path, skipped and empty tensors, param groups -- against torch's own
clip_grad_norm_ + Adam(foreach=False) and the reference's EMA expression on the CPU in float64, with the bar of
tests/optim_cases.py (3 x torch's own float32 error, per case and quantity, over all tensors of the case); the exact cases with
==; untouched memory around every tensor; independence of the list a tensor is in; repeatability; the version counters; the
EDM trainer's replay of the recorded reference run; and RNN.train_epoch with FusedAdam as a drop-in.  Every figure is printed
before it is held against its bar.

Measured on an MI355X: worst ratio to torch's own float32 error 2.01 over the 330 figures (bar 3); the trainer's replay 0.61
(losses), 0.98 (gradient norms), 1.00 (weights and EMA); the train_epoch drop-in 1.00."""
import copy

import numpy as np
import pytest
import torch

import ntm_amd
from ntm_amd import diffusion, optim
import diffusion_train_cases as C
import optim_cases as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -0x2AD5F00D          # the int32 pattern of the gaps (as a float: a large negative number)


def fused(case, **kw):
    return O.run(case, optim.FusedAdam, device=DEV, fused=True, **kw)


# ---- sizes and layouts, steps 1 - 3 with the state carried, the clip active / inactive / absent, p random / p = 0 -----------------------

@pytest.mark.parametrize("i,n", list(enumerate(O.ELEMENT_COUNTS)))
def test_element_counts_at_the_chunk_and_vector_edges(i, n):
    case = O.element_case(n, i)
    O.hold_case(f"n = {n} ({case.clip} clip)", case, fused(case))


@pytest.mark.parametrize("i,c", list(enumerate(O.TENSOR_COUNTS)))
def test_tensor_counts_at_the_table_edges(i, c):
    case = O.count_case(c, i)
    O.hold_case(f"{c} tensors ({case.clip} clip)", case, fused(case))


@pytest.mark.parametrize("clip,zero_p", [("active", False), ("inactive", True), ("absent", True)])
def test_a_mixed_list_with_a_missing_gradient_an_empty_parameter_and_two_groups(clip, zero_p):
    case = O.mixed_case(clip, zero_p)
    got = fused(case)
    assert got["stateless"] == [O.MAX - 5, len(case.sizes) // 2 + 2]        # .grad = None: no state, not in the norm
    O.hold_case(f"mixed list ({clip} clip, p {'= 0' if zero_p else 'random'})", case, got)


def test_lr_zero_keeps_the_parameters_and_advances_the_state():
    case = O.ramp_case()
    got = fused(case)
    assert not got["update"].any() and got["steps"] == [1.0] * 3 and got["exp_avg"].any() and got["exp_avg_sq"].any()
    O.hold_case("lr = 0", case, got)


def test_one_nan_gradient_element_reaches_every_parameter_as_in_torch():
    sizes = (5, O.CHUNK + 1, 3)
    ps = [torch.nn.Parameter(torch.ones(n, device=DEV)) for n in sizes]
    qs = [torch.nn.Parameter(torch.ones(n)) for n in sizes]
    for p, q in zip(ps, qs):
        q.grad = torch.ones_like(q)
    qs[1].grad[O.CHUNK - 7] = float("nan")
    for p, q in zip(ps, qs):
        p.grad = q.grad.to(DEV)
    norm = optim.FusedAdam(ps, **O.reference_hyper()).step(max_grad_norm=1.0)
    ref = torch.optim.Adam(qs, foreach=False, **O.reference_hyper())
    ref_norm = torch.nn.utils.clip_grad_norm_(qs, 1.0, foreach=False)
    ref.step()
    assert torch.isnan(ref_norm) and torch.isnan(norm)
    for p, q in zip(ps, qs):
        assert torch.isnan(q).all() and torch.isnan(p).all()


# ---- the exact cases ------------------------------------------------------------------------------------------------------------------

def test_exact_case_to_the_bit():
    O.assert_exact(O.exact_run(optim.FusedAdam, DEV, fused=True))


def test_exact_ema_to_the_bit():
    dst, src, want = O.ema_exact_case()
    d, s = [t.to(DEV) for t in dst], [t.to(DEV) for t in src]
    optim.ema_update_(d, s, 0.5)
    for got, w, q, orig in zip(d, want, s, src):
        assert torch.equal(got.cpu(), w) and torch.equal(q.cpu(), orig)


@pytest.mark.parametrize("s", [0.999, 0.004])
def test_ema_against_the_reference_expression(s):
    sizes = O.ELEMENT_COUNTS + O.small_sizes(O.MAX + 1)
    dst, src, up32, up64 = O.ema_case(sizes, s, 700)
    d, q = [t.to(DEV) for t in dst], [t.to(DEV) for t in src]
    optim.ema_update_(d, q, s)
    O.hold(f"ema update (s = {s})", O._cat([a.double().cpu() - b.double() for a, b in zip(d, dst)]), up32, up64)


# ---- memory and independence ----------------------------------------------------------------------------------------------------------

def arena_views(sizes, offsets):
    """One int32-sentinel arena; -> (arena, float32 views of `sizes` elements with sentinel gaps between them).  offsets[k]:
    elements to skip before view k on top of the rounding to 16 bytes -- 0: a 16-byte aligned view, 1: the scalar path."""
    starts, at = [], 4
    for n, off in zip(sizes, offsets):
        at = (at + 3) // 4 * 4 + off
        starts.append(at)
        at += n + 5
    arena = torch.full((at + 8,), SENTINEL, dtype=torch.int32, device=DEV)
    views = [arena.view(torch.float32)[a:a + n] for a, n in zip(starts, sizes)]
    assert all((v.data_ptr() % 16 == 0) == (off % 4 == 0) for v, off in zip(views, offsets))
    return arena, views


def gaps_of(arena, views):
    keep = torch.ones(arena.numel(), dtype=torch.bool, device=DEV)
    base = arena.data_ptr()
    for v in views:
        a = (v.data_ptr() - base) // 4
        keep[a:a + v.numel()] = False
    return arena[keep]


def test_nothing_is_written_outside_the_tensors_and_views_at_odd_offsets_work():
    """Parameters, gradients, state and EMA tensors are views into arenas with sentinel gaps; every second parameter and
    gradient sits at element offset 1 (the scalar path).  The state is preloaded through load_state_dict; three steps."""
    sizes = (1, 3, 4, 5, 255, 256, 257, O.CHUNK - 1, O.CHUNK, O.CHUNK + 1, 2 * O.CHUNK + 3, 7)
    K = len(sizes)
    offs = [k % 2 for k in range(K)]
    case = O.Case(sizes, seed=800, clip="active")
    arenas = {name: arena_views(sizes, o) for name, o in (("p", offs), ("g", offs[::-1]), ("m", [0] * K), ("v", offs), ("ema", offs))}
    P, G, M, V, E = (arenas[name][1] for name in ("p", "g", "m", "v", "ema"))
    # one earlier step on the CPU gives the state to preload and the parameters to start from, for the references too
    pre = [torch.nn.Parameter(p.clone()) for p in case.p0]
    opt0 = torch.optim.Adam(pre, foreach=False, **O.reference_hyper())
    for p, g in zip(pre, O.Case(sizes, seed=801, steps=1).grads[0]):
        p.grad = g
    opt0.step()
    pre = [p.detach().clone() for p in pre]
    sd = copy.deepcopy(opt0.state_dict())

    def continued(dtype):
        ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in pre]
        o = torch.optim.Adam(ps, foreach=False, **O.reference_hyper())
        o.load_state_dict(copy.deepcopy(sd))
        norms = []
        for gs in case.grads:
            for p, g in zip(ps, gs):
                p.grad = g.to(dtype).clone()
            norms.append(float(torch.nn.utils.clip_grad_norm_(ps, case.max_norm, foreach=False)))
            o.step()
        return {"update": O._cat([p.detach().double() - q.double() for p, q in zip(ps, pre)]),
                "exp_avg": O._cat([o.state[p]["exp_avg"] for p in ps]), "exp_avg_sq": O._cat([o.state[p]["exp_avg_sq"] for p in ps]),
                "grad": O._cat([p.grad for p in ps]), "norm": np.asarray(norms)}
    r32, r64 = continued(torch.float32), continued(torch.float64)
    assert np.all(r64["norm"] > case.max_norm)

    ps = []
    for k in range(K):
        P[k].copy_(pre[k])
        M[k].copy_(sd["state"][k]["exp_avg"])
        V[k].copy_(sd["state"][k]["exp_avg_sq"])
        E[k].copy_(case.p0[k])
        sd["state"][k]["exp_avg"], sd["state"][k]["exp_avg_sq"] = M[k], V[k]
        ps.append(torch.nn.Parameter(P[k]))
        ps[k].grad = G[k]
    opt = optim.FusedAdam(ps, **O.reference_hyper())
    opt.load_state_dict(sd)
    for k, p in enumerate(ps):                      # the views themselves, not copies
        assert p.data_ptr() == P[k].data_ptr() and p.grad.data_ptr() == G[k].data_ptr()
        assert opt.state[p]["exp_avg"].data_ptr() == M[k].data_ptr() and opt.state[p]["exp_avg_sq"].data_ptr() == V[k].data_ptr()
    norms = []
    for gs in case.grads:
        for k in range(K):
            G[k].copy_(gs[k])
        norms.append(float(opt.step(max_grad_norm=case.max_norm)))
    optim.ema_update_(E, ps, 0.75)
    for name, (arena, views) in arenas.items():
        gap = gaps_of(arena, views)
        assert gap.numel() >= 5 * K and bool((gap == SENTINEL).all()), f"the gaps of the {name} arena were written"
    assert [float(opt.state[p]["step"]) for p in ps] == [4.0] * K
    got = {"update": O._cat([p.detach().double().cpu() - q.double() for p, q in zip(ps, pre)]),
           "exp_avg": O._cat(M), "exp_avg_sq": O._cat(V), "grad": O._cat(G), "norm": np.asarray(norms)}
    for q in O.QUANTITIES:
        O.hold(f"arena {q}", got[q], r32[q], r64[q])
    ema32, ema64 = (O._cat([(e.to(dt) * 0.75 + p.detach().cpu().to(dt) * (1 - 0.75)).double() - e.double()
                            for e, p in zip(case.p0, ps)]) for dt in (torch.float32, torch.float64))
    O.hold("arena ema update", O._cat([a.double().cpu() - b.double() for a, b in zip(E, case.p0)]), ema32, ema64)


def test_a_tensor_does_not_depend_on_the_list_it_is_in():
    """Without a clip: entry k of a list of 2 MAX + 1 tensors, stepped alone, gives the same bits -- a wrong chunk-to-tensor map
    at a table boundary cannot."""
    count = 2 * O.MAX + 1
    sizes = list(O.small_sizes(count))
    for k, n in ((0, O.CHUNK + 1), (O.MAX - 1, 2 * O.CHUNK + 3), (O.MAX, 257), (O.MAX + 1, O.CHUNK), (2 * O.MAX, O.CHUNK - 1)):
        sizes[k] = n
    case = O.Case(sizes, seed=900, steps=2, clip="absent")

    def stepped(ks):
        ps = [torch.nn.Parameter(case.p0[k].to(DEV)) for k in ks]
        opt = optim.FusedAdam(ps, **O.reference_hyper())
        for gs in case.grads:
            for p, k in zip(ps, ks):
                p.grad = gs[k].to(DEV)
            assert opt.step() is None
        return [(p.detach().clone(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]) for p in ps]
    together = stepped(range(count))
    for k in (0, 1, O.MAX - 2, O.MAX - 1, O.MAX, O.MAX + 1, 2 * O.MAX - 1, 2 * O.MAX):
        for a, b in zip(stepped([k])[0], together[k]):
            assert torch.equal(a, b), k


def test_a_repeated_run_repeats_every_bit():
    case = O.mixed_case("active")
    a, b = fused(case), fused(case)
    for q in O.QUANTITIES:
        assert np.array_equal(a[q], b[q]), q


# ---- versions --------------------------------------------------------------------------------------------------------------------------

def test_version_counters_rise():
    ps = [torch.nn.Parameter(torch.randn(n, device=DEV)) for n in (5, 300)]
    ema = [torch.zeros(n, device=DEV) for n in (5, 300)]
    opt = optim.FusedAdam(ps)

    def versions():
        return [[t._version for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], p.grad)] for p in ps]
    for p in ps:
        p.grad = torch.randn_like(p)
    opt.step()                                  # the state is made here
    for clip in (None, 1.0):
        before = versions()
        opt.step(max_grad_norm=clip)
        for now, was in zip(versions(), before):
            assert all(n > o for n, o in zip(now[:3], was[:3])), (now, was)
            assert now[3] > was[3] if clip else now[3] == was[3]        # the gradient is written by the clip alone
    before, v0 = versions(), [e._version for e in ema]
    optim.ema_update_(ema, ps, 0.9)
    assert all(e._version > v for e, v in zip(ema, v0)) and versions() == before       # the sources are only read


def _net_with_gradients(seed):
    net = C.network(DEV)
    g = torch.Generator().manual_seed(seed)
    for p in net.parameters():
        if p.requires_grad:
            p.grad = (0.05 * torch.randn(p.shape, generator=g)).to(DEV)
    return net


def test_forward_follows_a_fused_step():
    net = _net_with_gradients(11).eval()
    g = torch.Generator().manual_seed(7)
    x, s = torch.randn(2, 512, generator=g).to(DEV), torch.tensor([[-0.9], [-1.4]], device=DEV)
    opt = optim.FusedAdam([p for p in net.parameters() if p.requires_grad], lr=1e-2)
    with torch.no_grad():
        first = net(x, s).clone()           # the packed copies and plans are made here
        opt.step(max_grad_norm=1.0)
        second = net(x, s).clone()
        fresh = diffusion.UNet1D(C.config(), DEV).eval()
        fresh.load_state_dict(net.state_dict())
        want = fresh(x, s)
    assert torch.equal(second, want) and not torch.equal(first, second)


def test_a_fused_step_between_forward_train_and_backward_is_caught():
    net = _net_with_gradients(12)
    g = torch.Generator().manual_seed(8)
    x, s = torch.randn(2, 512, generator=g).to(DEV), torch.tensor([[-0.9], [-1.4]], device=DEV)
    out = net.forward_train(x, s)
    optim.FusedAdam([p for p in net.parameters() if p.requires_grad]).step()
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        out.sum().backward()


# ---- EDMTrainer ------------------------------------------------------------------------------------------------------------------------

def test_edm_trainer_with_fused_adam_replays_the_reference_run():
    args, net = C.config(), C.network(DEV, torch.float32)
    hyper = dict(lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2), eps=args.train.optimizer.eps)
    tr = diffusion.EDMTrainer(args, net, optim.FusedAdam(net.parameters(), **hyper), DEV, backend="hip")
    a, r = C.arrays(), C.replay(tr, DEV, torch.float32)
    worst = {}
    C.hold("loss [three iterations]", np.asarray(r["loss"]), a["loss_ref32"], a["loss_ref64"], worst)
    C.hold("grad_norm [three iterations]", np.asarray(r["grad_norm"]), a["grad_norm_ref32"], a["grad_norm_ref64"], worst)
    assert r["lr"] == list(a["lr_ref64"])
    assert torch.is_tensor(tr.grad_norm) and tr.grad_norm.device.type == "cuda" and tr.grad_norm.dim() == 0
    for k in C.param_keys():
        C.hold(f"net [{k}]", r["net"][k], C.final("net", "32", k), C.final("net", "64", k), worst)
        C.hold(f"ema [{k}]", r["ema"][k], C.final("ema", "32", k), C.final("ema", "64", k), worst)
    print("worst ratio to the reference's own float32 error:", worst)
    # the checkpoint's optimizer entry moves to torch's Adam
    twin = C.network("cpu")
    theirs = torch.optim.Adam(twin.parameters(), **hyper)
    theirs.load_state_dict(copy.deepcopy(tr.state_dict()["optimizer"]))
    k0, p0 = next((k, p) for k, p in twin.named_parameters() if p.requires_grad)
    st = theirs.state[p0]
    assert float(st["step"]) == C.ITERS and st["exp_avg"].device.type == "cpu" and st["exp_avg"].any()
    assert torch.equal(st["exp_avg"], tr.optimizer.state[dict(tr.network.named_parameters())[k0]]["exp_avg"].cpu())
    for p in twin.parameters():
        p.grad = torch.ones_like(p)
    theirs.step()
    assert float(st["step"]) == C.ITERS + 1


# ---- the drop-in ------------------------------------------------------------------------------------------------------------------------

def test_rnn_train_epoch_takes_fused_adam_as_a_drop_in():
    """One epoch of RNN.train_epoch at hidden size 64: one stream, the warm-up and two windows.  The optimiser is under test, not
    the BPTT: the float64 and float32 CPU Adam are applied to the gradients that the run itself produced (a step pre-hook
    records them), and the parameters' update is held against the bar of the two."""
    torch.manual_seed(21)
    m = ntm_amd.RNN(1, 64, 1).cuda()
    init = [p.detach().cpu().clone() for p in m.parameters()]
    opt = optim.FusedAdam(m.parameters(), lr=1e-3)
    seen = []
    opt.register_step_pre_hook(lambda o, a, k: seen.append([p.grad.detach().cpu().clone() for p in m.parameters()]))
    g = torch.Generator().manual_seed(22)
    x = torch.rand(1, 1, 3 * 1024, generator=g) - 0.5
    loss = m.train_epoch([(x, 0.5 * x, None)], ntm_amd.ESRLoss(), opt)
    assert np.isfinite(loss) and len(seen) == 2

    def cpu_adam(dtype):
        ps = [torch.nn.Parameter(p.to(dtype).clone()) for p in init]
        o = torch.optim.Adam(ps, lr=1e-3, foreach=False)
        for gs in seen:
            for p, q in zip(ps, gs):
                p.grad = q.to(dtype).clone()
            o.step()
        return O._cat([p.detach().double() - q.double() for p, q in zip(ps, init)])
    got = O._cat([p.detach().double().cpu() - q.double() for p, q in zip(m.parameters(), init)])
    O.hold("RNN.train_epoch update", got, cpu_adam(torch.float32), cpu_adam(torch.float64))
