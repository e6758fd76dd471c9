"""GPU: the training path of the diffusion generators -- the adjoint of the fused ResnetBlock (csrc/unet_train.hip under
training.ResBlockFn), UNet1D.forward_train, EDMTrainer(backend="hip") and the stale-weights fix of UNet1D.forward.

The reference of the block tests is diffusion.ResnetBlock's own layers (g29 pins the module to the reference's class) on the
CPU under autograd, on the crop-and-concatenate input the kernel sees, in float64 (ref64) and float32 (ref32).  The bar of every
tensor is 3 x max|ref32 - ref64| / max|ref64| -- from the two references, never from the HIP result; a tensor whose ref64 is
identically zero must be exactly zero.  The network-level tests hold the same bar against the g30 goldens (the reference's own
training run) or against forward_torch.  Every figure is printed before it is held against its bar."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ntm_amd import diffusion
from ntm_amd.training import ResBlockFn
import diffusion_train_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda"
R2 = 2 ** 0.5
WORST = {}


def make_case(c0, c1, cout, T, n=8, off0=0, extra=0, init=False, B=2, seed=0):
    """Float32 operands of one block on the CPU: src0 (B, c0, T0) -- with init the waveform (B, 1, T0) --, src1, film (B, cin),
    the weights under ResnetBlock's default initialisation, init_w, gout."""
    g = torch.Generator().manual_seed(1000 + seed)
    cin, T0 = c0 + c1, T + off0 + extra
    torch.manual_seed(2000 + seed)
    blk = diffusion.ResnetBlock(cin, cout, 16, num_dils=n)
    op = {"src0": torch.randn(B, 1 if init else c0, T0, generator=g),
          "src1": torch.randn(B, c1, T, generator=g) if c1 else None,
          "film": 1 + 0.5 * torch.randn(B, cin, generator=g),
          "w_first": blk.first_conv[1].weight.detach().clone(),
          "w_gated": torch.stack([h.conv.weight.detach() for h in blk.H]).clone(),
          "w_res": None if cin == cout else blk.res_conv.weight.detach().clone(),
          "init_w": 0.5 * torch.randn(c0, 1, 5, generator=g) if init else None,
          "gout": torch.randn(B, cout, T, generator=g)}
    return op, dict(off0=off0, T=T, n=n)


def torch_block(op, meta, dt, dev="cpu"):
    """The module's arithmetic under autograd -> (out, [y_0 .. y_{n-1}], gradients by operand name; dW_l split per layer)."""
    t = {k: None if v is None else v.detach().to(dev, dt).clone().requires_grad_(k != "gout" and not (k == "src0" and op["init_w"] is not None))
         for k, v in op.items()}
    x0 = t["src0"] if t["init_w"] is None else F.conv1d(t["src0"], t["init_w"], padding="same")
    x = x0[:, :, meta["off0"]:meta["off0"] + meta["T"]]
    if t["src1"] is not None:
        x = torch.cat((x, t["src1"]), 1)
    x = x * t["film"].unsqueeze(-1)
    y, ys = F.conv1d(F.gelu(x), t["w_first"]), []
    for l in range(meta["n"]):
        ys.append(y)
        y = (y + F.conv1d(F.gelu(y), t["w_gated"][l], dilation=2 ** l, padding="same")) / R2
    out = (y + (x if t["w_res"] is None else F.conv1d(x, t["w_res"]))) / R2
    out.backward(t["gout"])
    grads = {k: v.grad for k, v in t.items() if v is not None and v.requires_grad}
    for l in range(meta["n"]):
        grads[f"w_gated.{l}"] = grads["w_gated"][l]
    del grads["w_gated"]
    return out.detach(), [v.detach() for v in ys], {k: v.detach() for k, v in grads.items()}


def hip_block(op, meta, need_src0=True):
    t = {k: None if v is None else v.detach().to(DEV).clone().requires_grad_(k != "gout" and not (k == "src0" and (op["init_w"] is not None or not need_src0)))
         for k, v in op.items()}
    out = ResBlockFn.apply(t["src0"], t["src1"], t["film"], t["w_first"], t["w_gated"], t["w_res"], t["init_w"], meta["off0"])
    ysave = out.grad_fn.saved_tensors[-1][:out.shape[0] * meta["n"] * out.shape[1] * meta["T"]].view(out.shape[0], meta["n"], out.shape[1], meta["T"])
    out.backward(t["gout"])
    grads = {k: v.grad for k, v in t.items() if v is not None and v.requires_grad}
    for l in range(meta["n"]):
        grads[f"w_gated.{l}"] = grads["w_gated"][l]
    del grads["w_gated"]
    return out.detach(), ysave.detach(), grads


def hold_block(name, op, meta):
    """Every output of the adjoint against the two references of this case."""
    _, _, g64 = torch_block(op, meta, torch.float64)
    _, _, g32 = torch_block(op, meta, torch.float32)
    _, _, got = hip_block(op, meta)
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    for k in sorted(g64):
        kind, _, layer = k.partition(".")
        C.hold(f"{kind} [{name}{' layer ' + layer if layer else ''}]", got[k], g32[k].numpy(), g64[k].numpy(), WORST)


T_EDGES = (1, 15, 16, 17, 255, 257, 512, 1000, 1024)
CHANNELS = {"identity 8-8": dict(c0=8, c1=0, cout=8), "8-16": dict(c0=8, c1=0, cout=16),
            "16+16-16": dict(c0=16, c1=16, cout=16), "16+16-16 cropped": dict(c0=16, c1=16, cout=16, off0=3, extra=4),
            "32-16": dict(c0=32, c1=0, cout=16), "5+3-12": dict(c0=5, c1=3, cout=12, off0=1, extra=2),
            "init 8-8": dict(c0=8, c1=0, cout=8, init=True), "init 8-16 cropped": dict(c0=8, c1=0, cout=16, init=True, off0=2)}
# (without a second source the block runs to the end of src0: only the two-source sets can leave frames behind the crop)


def test_forward_save_is_the_inference_forward_and_saves_every_layer_input():
    for name, T in (("16+16-16 cropped", 1000), ("5+3-12", 17), ("init 8-8", 512), ("identity 8-8", 1)):
        op, meta = make_case(T=T, seed=T, **CHANNELS[name])
        out, ysave, _ = hip_block(op, meta)
        d = {k: None if v is None else v.to(DEV) for k, v in op.items()}
        want = diffusion.resblock_forward(d["src0"], d["film"], d["w_first"], d["w_gated"], d["w_res"], d["src1"], meta["off0"],
                                          frames=T, init_w=d["init_w"], form="whole")
        assert torch.equal(out, want), name
        _, y64, _ = torch_block(op, meta, torch.float64)
        _, y32, _ = torch_block(op, meta, torch.float32)
        for l in range(meta["n"]):
            C.hold(f"y_save [{name} T={T} layer {l}]", ysave[:, l], y32[l].numpy(), y64[l].numpy(), WORST)


@pytest.mark.parametrize("T", T_EDGES)
def test_backward_at_every_frame_edge(T):
    op, meta = make_case(T=T, seed=T, **CHANNELS["16+16-16 cropped"])
    hold_block(f"16+16-16 cropped T={T}", op, meta)


@pytest.mark.parametrize("T", (17, 512))
@pytest.mark.parametrize("name", sorted(CHANNELS))
def test_backward_for_every_channel_set(name, T):
    op, meta = make_case(T=T, seed=T + len(name), **CHANNELS[name])
    hold_block(f"{name} T={T}", op, meta)


@pytest.mark.parametrize("name,T", [("8-16", 17), ("16+16-16 cropped", 257), ("init 8-8", 512)])
def test_backward_of_a_single_layer(name, T):
    op, meta = make_case(T=T, n=1, seed=7 * T, **CHANNELS[name])
    hold_block(f"{name} n=1 T={T}", op, meta)


def test_streams_are_independent_and_calls_repeat_bit_for_bit():
    op, meta = make_case(T=300, B=3, seed=5, **CHANNELS["16+16-16 cropped"])
    _, _, whole = hip_block(op, meta)
    _, _, again = hip_block(op, meta)
    for k in whole:
        assert torch.equal(whole[k], again[k]), k               # the reduced weight gradients among them
    for b in range(3):
        one = {k: v[b:b + 1] if v is not None and k in ("src0", "src1", "film", "gout") else v for k, v in op.items()}
        _, _, got = hip_block(one, meta)
        for k in ("src0", "src1", "film"):
            assert torch.equal(got[k], whole[k][b:b + 1]), (k, b)
    _, _, without = hip_block(op, meta, need_src0=False)         # g_src0 == NULL
    assert "src0" not in without
    for k in without:
        assert torch.equal(without[k], whole[k]), k
    # one FiLM row for all streams: its gradient is the sum of the per-stream rows
    shared = dict(op, film=op["film"][:1])
    _, _, g64 = torch_block(shared, meta, torch.float64)
    _, _, g32 = torch_block(shared, meta, torch.float32)
    _, _, got = hip_block(shared, meta)
    assert got["film"].shape == (1, 32)
    C.hold("film [one row for three streams]", got["film"], g32["film"].numpy(), g64["film"].numpy(), WORST)


def integer_gout(shape, gen):
    """gout whose product with the kernel's float32 1 / sqrt 2 rounds to a small integer exactly: go = gout / sqrt 2 is then an
    integer operand, as the weights and inputs of the exact case are."""
    c = np.float32(0.70710678118654752440)
    table = {}
    for k in range(-4, 5):           # the float32 next to k sqrt 2 whose product rounds to k, where there is one
        g = np.float32(k * R2)
        for cand in (g, np.nextafter(g, np.float32(np.inf)), np.nextafter(g, np.float32(-np.inf))):
            if np.float32(cand * c) == np.float32(k):
                table[k] = cand
                break
    have = sorted(table)
    assert len(have) >= 5 and have[0] < 0 < have[-1], have
    ks = torch.tensor(have)[torch.randint(0, len(have), shape, generator=gen)]
    return torch.from_numpy(np.vectorize(table.get, otypes=[np.float32])(ks.numpy())), ks


@pytest.mark.parametrize("name", ["16+16-16 cropped", "identity 8-8", "init 8-16 cropped"])
def test_exact_integer_linear_tail(name):
    """Small-integer inputs, FiLM, W_res, init_w and gout / sqrt 2, with W_first and the gated weights zero (the entry point takes
    at least one gated layer; zero weights leave gy_0 out of gX): every product and sum of the linear tail is exact in fp32, so
    dW_res, dinit_w, gfilm and g_src must EQUAL the integer result.  dW_first = gy_0 gelu(X)^T is on the gelu path and is not
    checked here."""
    kw, T, B = CHANNELS[name], 200, 2
    gen = torch.Generator().manual_seed(99)
    op, meta = make_case(T=T, n=1, B=B, seed=3, **kw)
    ints = lambda t, lo, hi: None if t is None else torch.randint(lo, hi + 1, t.shape, generator=gen).float()      # noqa: E731
    op.update(src0=ints(op["src0"], -3, 3), src1=ints(op["src1"], -3, 3), film=ints(op["film"], -2, 2),
              w_res=ints(op["w_res"], -2, 2), init_w=ints(op["init_w"], -2, 2), w_first=torch.zeros_like(op["w_first"]),
              w_gated=torch.zeros_like(op["w_gated"]))
    op["gout"], go = integer_gout(op["gout"].shape, gen)
    _, _, got = hip_block(op, meta)
    # the integer result, in int64
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
    c0 = kw["c0"]
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


@pytest.fixture(scope="module")
def hip_replay():
    return C.replay(C.trainer(DEV, torch.float32, "hip"), DEV, torch.float32)


def test_forward_train_output_and_gradients_against_the_reference_run(hip_replay):
    a, tr = C.arrays(), C.trainer(DEV, torch.float32, "hip")
    x, (u, noise) = C.batch(0, DEV)
    sigma = tr.sample_ptrain_safe(C.B, u).unsqueeze(-1).to(DEV)
    inputs, _, cnoise = tr.prepare_train_preconditioning(x, sigma, noise)
    out = tr.network.forward_train(inputs, cnoise)
    assert out.requires_grad and out.shape == (C.B, C.T)
    C.hold("net_out [forward_train, iteration 0]", out, a["net_out_ref32"], a["net_out_ref64"], WORST)
    assert sorted(hip_replay["grads"]) == sorted(C.trained_keys())
    for k in C.trained_keys():
        C.hold(f"param_grad [{k}]", hip_replay["grads"][k], a["grad32_" + k], a["grad64_" + k], WORST)


def test_trainer_on_the_hip_backend_replays_the_reference_run(hip_replay):
    a, r = C.arrays(), hip_replay
    C.hold("loss [three iterations]", np.asarray(r["loss"]), a["loss_ref32"], a["loss_ref64"], WORST)
    assert r["lr"] == list(a["lr_ref64"])
    for k in C.param_keys():
        C.hold(f"net [{k}]", r["net"][k], C.final("net", "32", k), C.final("net", "64", k), WORST)
        C.hold(f"ema [{k}]", r["ema"][k], C.final("ema", "32", k), C.final("ema", "64", k), WORST)


def test_forward_follows_an_in_place_update_of_the_parameters():
    net = C.network(DEV).eval()
    g = torch.Generator().manual_seed(7)
    x, s = torch.randn(2, 512, generator=g).to(DEV), torch.tensor([[-0.9], [-1.4]], device=DEV)
    with torch.no_grad():
        first = net(x, s).clone()
        net.downs[1][0].H[3].conv.weight.add_(0.05)
        net.middle[0][0].film.output_layer.weight.add_(0.1)
        second = net(x, s).clone()
        fresh = diffusion.UNet1D(C.config(), DEV).eval()
        fresh.load_state_dict(net.state_dict())
        want = fresh(x, s)
    assert torch.equal(second, want) and not torch.equal(first, second)


def test_noise_shaped_net_trains_with_its_long_levels_in_torch():
    args = diffusion.load_config("noise")
    args.network.depth, T = 6, 4096
    torch.manual_seed(31)
    ref = diffusion.UNet1D(args, "cpu")
    for m in ref.modules():
        if isinstance(m, diffusion.CombinerUp):
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
    g = torch.Generator().manual_seed(32)
    x, s, gout = torch.randn(1, T, generator=g), torch.tensor([[-1.5]]), torch.randn(1, T, generator=g)

    def grads(net, dev, dt, method):
        net = net.to(dev, dt)
        net.zero_grad()
        out = getattr(net, method)(x.to(dev, dt), s.to(dev, dt))
        (out * gout.to(dev, dt)).sum().backward()
        return out.detach(), {k: p.grad.detach().cpu() for k, p in net.named_parameters() if p.grad is not None}

    calls = []
    orig = ResBlockFn.apply
    o64, g64 = grads(copy.deepcopy(ref), "cpu", torch.float64, "forward_torch")
    o32, g32 = grads(copy.deepcopy(ref), "cpu", torch.float32, "forward_torch")
    ResBlockFn.apply = staticmethod(lambda *a: (calls.append(a[0].shape[2]), orig(*a))[1])
    try:
        out, got = grads(copy.deepcopy(ref), DEV, torch.float32, "forward_train")
    finally:
        ResBlockFn.apply = orig
    # the 4096-frame level runs the torch modules, every shorter one the HIP node
    assert sorted(set(calls)) == [4, 16, 64, 256, 1024] and len(calls) == 11, calls
    C.hold("net_out [noise-shaped, T=4096]", out, o32.numpy(), o64.numpy(), WORST)
    assert sorted(got) == sorted(g64)
    for k in sorted(g64):
        C.hold(f"param_grad [noise-shaped {k}]", got[k], g32[k].numpy(), g64[k].numpy(), WORST)


def test_zz_report_worst_ratios():
    print("worst ratio to the reference's own float32 error, per kind of tensor:", {k: f"{v:.2f}" for k, v in sorted(WORST.items())})
