"""GPU: the adjoints of the resample + combine steps of the diffusion generators' UNet1D (csrc/unet_resample_train.hip under
training.DownCombineFn / UpCombineFn), diffusion.down_combine / up_combine as differentiable functions, and UNet1D.forward_train
on these nodes.

The reference and the bound are resample_adjoint_cases': float64 torch autograd of the torch modules on the CPU, and
|got - ref64| <= N 2^-24 A elementwise with A the same computation on absolute values -- derived from the arithmetic, never from
the HIP result (tests/test_resample_adjoint_cpu.py pins the case module).  Every worst fraction is printed before it is held."""
import numpy as np
import pytest
import torch

from ntm_amd import diffusion
from ntm_amd.training import DownCombineFn, UpCombineFn
import diffusion_train_cases as C
import resample_adjoint_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}


def hip_step(case, op, w, grads="both", need=("x", "pyr", "wc"), fn=None):
    """One node, forward and backward, on the device -> dict(xo, po, g_x, g_pyr, g_wc); `need`: the operands that require a
    gradient (an absent one maps to a null output pointer); fn: the public function instead of the node."""
    t = {k: None if v is None else v.detach().to(DEV).clone() for k, v in op.items()}
    for k in need:
        if t[k] is not None:
            t[k].requires_grad_(True)
    down = case["kind"] == "down"
    if fn is None:
        fn = DownCombineFn.apply if down else UpCombineFn.apply
    xo, po = fn(t["x"], t["pyr"], t["ker"], t["wc"], case["S"], w)
    loss = 0
    if grads in ("both", "xo") and xo is not None:
        loss = loss + (xo * t["g_xo"]).sum()
    if grads in ("both", "po"):
        loss = loss + (po * t["g_po"]).sum()
    loss.backward()
    return {"xo": None if xo is None else xo.detach(), "po": po.detach(), "g_x": t["x"].grad,
            "g_pyr": None if t["pyr"] is None else t["pyr"].grad, "g_wc": t["wc"].grad}


def hold(name, case, got, grads="both"):
    ref, A = R.reference(name, grads)
    N = R.n_roundings(case["kind"], case["S"], case["C"])
    for k in ("g_x", "g_pyr", "g_wc"):
        if ref[k] is None:
            assert got[k] is None, (name, k)
            continue
        assert got[k] is not None and got[k].dtype == torch.float32, (name, grads, k)
        fr = R.fraction(got[k], ref[k], A[k], N)
        key = f"{case['kind']} {k}"
        WORST[key] = max(WORST.get(key, 0.0), fr)
        print(f"{name} [{grads}] {k}: {fr:.4f} of the bound (N = {N})")
        assert fr <= 1.0, (name, grads, k, fr)


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_gradients_hold_the_derived_bound(name):
    case = R.CASES[name]
    op, w = R.operands(case)
    for grads in R.variants(case):
        hold(name, case, hip_step(case, op, w, grads), grads)


@pytest.mark.parametrize("name", ["down S=4 F=257 C=5 pyr=0", "down S=3 F=1000 C=16 pyr=0", "up S=4 F=257 C=5 pyr=3",
                                  "up S=2 F=257 C=5 pyr=None", "up S=1 F=257 C=5 pyr=0", "up S=3 F=3 C=5 pyr=None"])
def test_forward_is_the_inference_launch_and_the_functions_route_through_the_nodes(name):
    case = R.CASES[name]
    op, w = R.operands(case)
    d = {k: None if v is None else v.to(DEV) for k, v in op.items()}
    fn = diffusion.down_combine if case["kind"] == "down" else diffusion.up_combine
    with torch.no_grad():
        want = fn(d["x"], d["pyr"], d["ker"], d["wc"], case["S"], w)
    plain = fn(d["x"], d["pyr"], d["ker"], d["wc"], case["S"], w)            # nothing requires a gradient: as before
    assert all(o is None or not o.requires_grad for o in plain)
    node = hip_step(case, op, w)
    public = hip_step(case, op, w, fn=fn)
    for i, k in enumerate(("xo", "po")):
        if want[i] is None:
            assert node[k] is None and public[k] is None and plain[i] is None
            continue
        assert torch.equal(node[k], want[i]) and torch.equal(public[k], want[i]) and torch.equal(plain[i], want[i]), (name, k)
    for k in ("g_x", "g_pyr", "g_wc"):                                        # the function is the node
        assert (node[k] is None and public[k] is None) or torch.equal(node[k], public[k]), (name, k)
    hold(name, case, public)


@pytest.mark.parametrize("name", ["down S=4 F=257 C=5 pyr=0", "down S=2 F=1000 C=16 pyr=0", "up S=4 F=257 C=5 pyr=3",
                                  "up S=3 F=257 C=5 pyr=0", "up S=1 F=257 C=5 pyr=0"])
def test_each_output_is_optional_and_the_others_keep_their_bits(name):
    case = R.CASES[name]
    op, w = R.operands(case)
    whole = hip_step(case, op, w)
    out_of = {"x": "g_x", "pyr": "g_pyr", "wc": "g_wc"}
    for leave in ("x", "pyr", "wc"):
        need = tuple(k for k in out_of if k != leave)
        got = hip_step(case, op, w, need=need)
        assert got[out_of[leave]] is None
        for k in need:
            assert torch.equal(got[out_of[k]], whole[out_of[k]]), (name, leave, k)
    only = hip_step(case, op, w, need=("wc",))                               # the combiner weight alone
    assert only["g_x"] is None and only["g_pyr"] is None and torch.equal(only["g_wc"], whole["g_wc"])


@pytest.mark.parametrize("name", sorted(R.EXACT))
def test_exact_integer_cases(name):
    """Small-integer operands, the filter among them, where no 1 / sqrt 2 enters: the results must EQUAL the int64 gather."""
    case = R.EXACT[name]
    op, w = R.integer_operands(case)
    grads = "po" if case["kind"] == "down" else "both"
    got = hip_step(case, op, w, grads)
    want = R.numpy_step(case, op, w, grads, dtype=np.int64)
    for k in (("g_pyr",) if case["kind"] == "down" else ("g_x", "g_wc")):
        assert np.any(want[k]) and torch.equal(got[k].cpu().double(), torch.from_numpy(want[k]).double()), (name, k)
    if case["kind"] == "down":                                               # nothing reaches x or the weight through po
        assert not got["g_x"].any() and not got["g_wc"].any()


@pytest.mark.parametrize("name", ["down S=4 F=1000 C=16 pyr=0", "down S=3 F=257 C=5 pyr=0", "up S=4 F=1000 C=16 pyr=0",
                                  "up S=2 F=257 C=5 pyr=None", "up S=1 F=257 C=5 pyr=3"])
def test_streams_are_independent_and_calls_repeat_bit_for_bit(name):
    case = dict(R.CASES[name], B=3)
    op, w = R.operands(case, seed=1)
    whole, again = hip_step(case, op, w), hip_step(case, op, w)
    for k in ("g_x", "g_pyr", "g_wc"):
        assert (whole[k] is None and again[k] is None) or torch.equal(whole[k], again[k]), (name, k)
    for b in range(3):
        one = {k: v[b:b + 1] if v is not None and k in ("x", "pyr", "g_xo", "g_po") else v for k, v in op.items()}
        got = hip_step(dict(case, B=1), one, w)
        for k in ("g_x", "g_pyr"):
            assert (whole[k] is None and got[k] is None) or torch.equal(got[k], whole[k][b:b + 1]), (name, k, b)


@pytest.mark.parametrize("name", sorted(R.LONG))
def test_a_long_level_holds_the_bound(name):
    """F = 65 536 at C = 16, S = 4: the noise net's top level, the longest fp64 partial."""
    case = R.LONG[name]
    op, w = R.operands(case)
    hold(name, case, hip_step(case, op, w))


def walk(fn, seen=None):
    seen = {} if seen is None else seen
    stack = [fn]
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen[f] = type(f).__name__
        stack.extend(n for n, _ in f.next_functions)
    return list(seen.values())


@pytest.fixture(scope="module")
def net_and_input():
    net = C.network(DEV)
    for m in net.modules():                      # CombinerUp starts at zero: its input would then take no gradient
        if isinstance(m, diffusion.CombinerUp):
            torch.manual_seed(11)
            torch.nn.init.kaiming_uniform_(m.conv1x1.weight, a=5 ** 0.5)
    x, _ = C.batch(0, DEV)
    return net, x, torch.tensor([[-0.7], [-1.1], [-1.6], [-2.2]], device=DEV)


def test_the_network_graph_holds_the_nodes_and_no_convolution(net_and_input):
    net, x, s = net_and_input
    out = net.forward_train(x, s)
    names = walk(out.grad_fn)
    assert names.count("DownCombineFnBackward") == 3 and names.count("UpCombineFnBackward") == 4, sorted(set(names))
    assert not [n for n in names if n.startswith("Convolution")], sorted(set(names))
    assert names.count("ResBlockFnBackward") == 9


def test_record_reports_the_names_and_values_of_forward_torch(net_and_input):
    net, x, s = net_and_input
    got, ref = {}, {}
    out = net.forward_train(x, s, record=lambda n, t: got.__setitem__(n, t.detach().cpu()))
    cpu64, cpu32 = C.network("cpu", torch.float64), C.network("cpu", torch.float32)
    for tag, ref_net, dt in (("64", cpu64, torch.float64), ("32", cpu32, torch.float32)):
        ref_net.load_state_dict({k: v.cpu().to(dt) if v.is_floating_point() else v.cpu() for k, v in net.state_dict().items()})
        with torch.no_grad():
            ref_net.forward_torch(x.cpu().to(dt), s.cpu().to(dt), record=lambda n, t, tag=tag: ref.__setitem__((n, tag), t.numpy()))
    assert list(got) == [n for n, tag in ref if tag == "64"] and torch.equal(got["final"], out.detach().cpu())
    for n in got:
        C.hold(f"record [{n}]", got[n], ref[(n, "32")], ref[(n, "64")])


def test_zz_report_worst_fractions():
    print("worst fraction of the derived bound per output:", {k: f"{v:.4f}" for k, v in sorted(WORST.items())})
