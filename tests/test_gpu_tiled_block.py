"""GPU: the training of the tiled ResnetBlock -- the forward with save and the adjoint on windows of a tile of 512 frames and
256 of halo a side (csrc/unet_train.hip under training.ResBlockTiledFn) -- and the noise-shaped network and its trainer on it.

The reference of the block tests is diffusion.ResnetBlock's own layers on the CPU under autograd, on the crop-and-concatenate
input the kernel sees, in float64 (ref64) and float32 (ref32).  The bar of every tensor is 3 x max|ref32 - ref64| / max|ref64|
-- from the two references, never from the HIP result; a tensor whose ref64 is identically zero must be exactly zero.  The
network-level tests hold the same bar against forward_torch / the torch backend on the CPU.  Every figure is printed before it
is held against its bar."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ntm_amd import diffusion
from ntm_amd import training
import tiled_block_cases as C

pytestmark = pytest.mark.gpu
DEV = C.DEV
WORST = {}


def hold_block(tag, name, T, n=8, seed=None):
    """Every output of the adjoint against the two references of this case."""
    seed = T if seed is None else seed
    op, meta = C.make_case(name, T, n, 2, seed)
    (_, _, g64), (_, _, g32) = C.reference(name, T, n, 2, seed)
    _, _, got = C.hip_block(op, meta)
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    for k in sorted(g64):
        kind, _, layer = k.partition(".")
        C.hold(f"{kind} [{tag} {name} T={T} n={n}{' layer ' + layer if layer else ''}]", got[k], g32[k].numpy(), g64[k].numpy(), WORST)


@pytest.mark.parametrize("name,T", [("16+16-16 cropped", 513), ("16+16-16 cropped", 1537), ("init 8-16 cropped", 1300)])
def test_forward_save_is_the_tiled_inference_forward_and_saves_every_layer_input(name, T):
    op, meta = C.make_case(name, T, 8, 2, T)
    out, ysave, _ = C.hip_block(op, meta)
    d = {k: None if v is None else v.to(DEV) for k, v in op.items()}
    want = diffusion.resblock_forward(d["src0"], d["film"], d["w_first"], d["w_gated"], d["w_res"], d["src1"], meta["off0"],
                                      frames=T, init_w=d["init_w"], form="tiled")
    assert torch.equal(out, want), name
    (_, y64, _), (_, y32, _) = C.reference(name, T, 8, 2, T)
    for l in range(meta["n"]):
        C.hold(f"y_save [{name} T={T} layer {l}]", ysave[:, l], y32[l].numpy(), y64[l].numpy(), WORST)


# forced tiled below the whole form's limit: one tile, a second tile of one frame, halos that leave the signal on both sides
@pytest.mark.parametrize("T", (1, 17, 511, 512, 513, 768, 1024))
def test_backward_forced_tiled_at_every_tile_edge(T):
    hold_block("forced", "16+16-16 cropped", T)


# what the auto form picks: three tiles and more, a middle tile with full halos
@pytest.mark.parametrize("T", (1025, 1536, 1537, 2049))
def test_backward_auto_above_the_whole_form(T):
    hold_block("auto", "16+16-16 cropped", T)


@pytest.mark.parametrize("name,T", [("identity 8-8", 513), ("identity 8-8", 1537), ("5+3-12", 17), ("5+3-12", 1025),
                                    ("init 8-16 cropped", 768), ("init 8-16 cropped", 1536)])
def test_backward_for_every_channel_set(name, T):
    hold_block("set", name, T, seed=T + len(name))


# one run at its full reach of 254 frames (seven layers), a single layer, and the two runs of eight layers at other sets
@pytest.mark.parametrize("name,T,n", [("16+16-16 cropped", 1537, 7), ("5+3-12", 513, 7), ("identity 8-8", 1025, 1),
                                      ("init 8-16 cropped", 513, 1), ("5+3-12", 2049, 8)])
def test_backward_for_every_split_into_runs(name, T, n):
    hold_block("runs", name, T, n, seed=7 * T + n)


def test_every_seam_holds_the_bar_on_its_own():
    """g_src0 / g_src1 on a band of 300 frames either side of every multiple of 256 (the tile and halo edges), each band against
    the bar of its own values: a wrong halo must not hide under a large value elsewhere."""
    name, T = "16+16-16 cropped", 2049
    op, meta = C.make_case(name, T, 8, 2, T)
    (_, _, g64), (_, _, g32) = C.reference(name, T, 8, 2, T)
    _, _, got = C.hip_block(op, meta)
    for m in range(0, T + 1, 256):
        lo, hi = max(0, m - 300), min(T, m + 300)
        for k, off in (("src0", meta["off0"]), ("src1", 0)):
            s = slice(off + lo, off + hi)
            C.hold(f"{k}_seam [around frame {m}]", got[k][:, :, s], g32[k][:, :, s].numpy(), g64[k][:, :, s].numpy(), WORST)


def test_streams_are_independent_and_calls_repeat_bit_for_bit():
    name, T = "16+16-16 cropped", 1537
    op, meta = C.make_case(name, T, 8, 3, 5)
    _, _, whole = C.hip_block(op, meta)
    _, _, again = C.hip_block(op, meta)
    for k in whole:
        assert torch.equal(whole[k], again[k]), k               # the reduced weight gradients among them
    for b in range(3):
        one = {k: v[b:b + 1] if v is not None and k in ("src0", "src1", "film", "gout") else v for k, v in op.items()}
        _, _, got = C.hip_block(one, meta)
        for k in ("src0", "src1", "film"):
            assert torch.equal(got[k], whole[k][b:b + 1]), (k, b)
    for left_out in ("src0", "src1"):                            # g_src0 == NULL, g_src1 == NULL
        _, _, without = C.hip_block(op, meta, skip=(left_out,))
        assert left_out not in without and len(without) == len(whole) - 1
        for k in without:
            assert torch.equal(without[k], whole[k]), (left_out, k)
    # one FiLM row for all streams: its gradient is the sum of the per-stream rows
    shared = dict(op, film=op["film"][:1])
    _, _, g64 = C.torch_block(shared, meta, torch.float64)
    _, _, g32 = C.torch_block(shared, meta, torch.float32)
    _, _, got = C.hip_block(shared, meta)
    assert got["film"].shape == (1, 32)
    C.hold("film [one row for three streams]", got["film"], g32["film"].numpy(), g64["film"].numpy(), WORST)


@pytest.mark.parametrize("name", ["16+16-16 cropped", "identity 8-8", "init 8-16 cropped"])
def test_exact_integer_linear_tail(name):
    """Small-integer inputs, FiLM, W_res, init_w and gout / sqrt 2, with W_first and the gated weights zero: every product and sum
    of the linear tail is exact in fp32 (the largest sum, dinit_w's, stays below 2^22), through four tiles and the fixed-order
    sums over them, so dW_res, dinit_w, gfilm and g_src must EQUAL the integer result."""
    T, B = 1537, 2
    gen = torch.Generator().manual_seed(99)
    op, meta = C.make_case(name, T, 1, B, 3)
    op = dict(op)
    ints = lambda t, lo, hi: None if t is None else torch.randint(lo, hi + 1, t.shape, generator=gen).float()      # noqa: E731
    op.update(src0=ints(op["src0"], -3, 3), src1=ints(op["src1"], -3, 3), film=ints(op["film"], -2, 2),
              w_res=ints(op["w_res"], -2, 2), init_w=ints(op["init_w"], -2, 2), w_first=torch.zeros_like(op["w_first"]),
              w_gated=torch.zeros_like(op["w_gated"]))
    op["gout"], go = C.integer_gout(op["gout"].shape, gen)
    _, _, got = C.hip_block(op, meta)
    i = {k: None if v is None else v.long() for k, v in op.items() if k != "gout"}
    if i["init_w"] is None:
        x0 = i["src0"]
    else:
        x0 = F.conv1d(op["src0"].double(), op["init_w"].double(), padding="same").long()
    xin = x0[:, :, meta["off0"]:meta["off0"] + T]
    if i["src1"] is not None:
        xin = torch.cat((xin, i["src1"]), 1)
    X = xin * i["film"].unsqueeze(-1)
    gX = go if i["w_res"] is None else torch.einsum("oc,bot->bct", i["w_res"][:, :, 0], go)
    gxin = gX * i["film"].unsqueeze(-1)
    c0 = meta["c0"]
    assert torch.equal(got["film"].cpu().long(), (gX * xin).sum(2)) and torch.equal(got["film"].cpu(), got["film"].cpu().round())
    if i["w_res"] is not None:
        assert torch.equal(got["w_res"].cpu()[:, :, 0].double(), torch.einsum("bot,bct->oc", go, X).double())
    if i["src1"] is not None:
        assert torch.equal(got["src1"].cpu().double(), gxin[:, c0:].double())
    if i["init_w"] is None:
        want = torch.zeros_like(op["src0"], dtype=torch.float64)
        want[:, :, meta["off0"]:meta["off0"] + T] = gxin[:, :c0].double()
        assert torch.equal(got["src0"].cpu().double(), want)
    else:
        raw = F.pad(i["src0"][:, 0], (2, 2))
        want = torch.stack([(gxin[:, :c0] * raw[:, None, meta["off0"] + k:meta["off0"] + k + T]).sum((0, 2)) for k in range(5)], 1)
        assert torch.equal(got["init_w"].cpu()[:, 0].double(), want.double())


def graph_nodes(fn):
    seen, stack = set(), [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        stack.extend(g for g, _ in f.next_functions)
    return sorted({type(f).__name__ for f in seen})


def test_noise_shaped_net_trains_with_every_block_on_the_device():
    """T = 5000: the levels are 5000, 1250, 313, 79, 20, 5 and 2 frames -- two tiled levels, with odd crops on the way up."""
    T, B = 5000, 2
    ref = C.noise_net()
    g = torch.Generator().manual_seed(32)
    x, s, gout = torch.randn(B, T, generator=g), torch.tensor([[-1.5], [-0.8]]), torch.randn(B, T, generator=g)

    def grads(net, dev, dt, method, look=None):
        net = net.to(dev, dt)
        net.zero_grad()
        out = getattr(net, method)(x.to(dev, dt), s.to(dev, dt))
        if look is not None:
            look.extend(graph_nodes(out.grad_fn))
        (out * gout.to(dev, dt)).sum().backward()
        return out.detach(), {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}

    o64, g64 = grads(copy.deepcopy(ref), "cpu", torch.float64, "forward_torch")
    o32, g32 = grads(copy.deepcopy(ref), "cpu", torch.float32, "forward_torch")
    calls, nodes = [], []
    orig = training.ResBlockTiledFn.apply
    training.ResBlockTiledFn.apply = staticmethod(lambda *a: (calls.append((a[1] if a[1] is not None else a[0]).shape[2]), orig(*a))[1])
    try:
        out, got = grads(copy.deepcopy(ref), DEV, torch.float32, "forward_train", nodes)
    finally:
        training.ResBlockTiledFn.apply = orig
    assert sorted(calls) == [1250, 1250, 5000, 5000], calls      # a block down and a block up at each of the two long levels
    assert nodes and not [n for n in nodes if "Convolution" in n], nodes
    C.hold("net_out [noise-shaped, T=5000]", out, o32.numpy(), o64.numpy(), WORST)
    assert sorted(got) == sorted(g64)
    for k in sorted(g64):
        C.hold(f"param_grad [noise-shaped {k}]", got[k], g32[k].numpy(), g64[k].numpy(), WORST)


def test_trainer_iteration_on_the_noise_shaped_net():
    """One EDMTrainer iteration at B = 2 x 4096 with recorded draws, at it = 1 (the ramp starts from a learning rate of 0 at
    it = 0, which would leave the weights where they were)."""
    T, B = 4096, 2
    args = C.noise_config()
    g = torch.Generator().manual_seed(41)
    x = args.diff_params.sigma_data * torch.randn(B, T, generator=g)
    draws = (torch.rand(B, generator=g), torch.randn(B, T, generator=g))

    def run(dev, dt, backend):
        net = copy.deepcopy(C.noise_net()).to(dev, dt)
        opt = torch.optim.Adam(net.parameters(), lr=args.train.lr, betas=(args.train.optimizer.beta1, args.train.optimizer.beta2),
                               eps=args.train.optimizer.eps)
        tr = diffusion.EDMTrainer(args, net, opt, dev, backend=backend)
        tr.it = 1
        loss = float(tr.iteration(x.to(dev, dt), tuple(d.to(dt) for d in draws)))
        assert tr.lr == args.train.lr / args.train.lr_rampup_it
        return loss, float(tr.grad_norm), {k: p.detach().double().cpu().numpy() for k, p in net.named_parameters()}

    l64, n64, w64 = run("cpu", torch.float64, "torch")
    l32, n32, w32 = run("cpu", torch.float32, "torch")
    loss, norm, w = run(DEV, torch.float32, "hip")
    C.hold("loss [one iteration, noise-shaped]", np.asarray([loss]), np.asarray([l32]), np.asarray([l64]), WORST)
    C.hold("grad_norm [one iteration, noise-shaped]", np.asarray([norm]), np.asarray([n32]), np.asarray([n64]), WORST)
    for k in sorted(w64):
        C.hold(f"net [{k}]", w[k], w32[k], w64[k], WORST)


def test_zz_report_worst_ratios():
    print("worst ratio to the reference's own float32 error, per kind of tensor:", {k: f"{v:.2f}" for k, v in sorted(WORST.items())})
