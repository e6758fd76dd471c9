"""CPU: the host side of the adversarial run -- ntm_amd.adversarial.load_config against the reference's own table (golden g28),
the two ntm_adv_head entry points in the header and the binding, ntm_amd.evaluation.val_loss_supervised's running-sum protocol,
tools/train_adversarial.py's command line, and the refusals that need no device."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import ntm_amd
from helpers import GOLDEN, ROOT

CONFIGS = (0, 1, 2, 3, 4, 5, 6, 7, 10)
SYMS = ("ntm_adv_head_forward", "ntm_adv_head_backward")
KEYS = ("ms_spec_loss", "ms_log_spec_loss", "mel_spec_loss", "log_mel_spec_loss", "ESR", "MSE", "ESRDCPre")


def tool():
    spec = importlib.util.spec_from_file_location("train_adversarial", os.path.join(ROOT, "tools", "train_adversarial.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_load_config_is_the_reference_s_table():
    table = json.load(open(os.path.join(GOLDEN, "g28_adversarial_configs.json")))
    assert sorted(int(n) for n in table) == sorted(CONFIGS) == sorted(ntm_amd.adversarial.CONFIGS)
    for n in CONFIGS:
        got = ntm_amd.adversarial.load_config(n)
        assert got == table[str(n)], n
        assert list(got) == ["segment_length", "tbptt_length", "val_segment_length", "gen_lr", "val_freq", "hid_size", "batch_size",
                             "model_path", "dataset_path", "crit", "crit_pars", "crit_lr"]
        # a fresh dict per call: get_critic writes test_in_len into crit_pars
        got["crit_pars"]["test_in_len"] = 1
        assert "test_in_len" not in ntm_amd.adversarial.load_config(n)["crit_pars"]
    for bad in (8, 9, 11, -1, "10", 1.0, True):
        with pytest.raises(ValueError, match="0, 1, 2, 3, 4, 5, 6, 7, 10"):
            ntm_amd.adversarial.load_config(bad)


def test_the_head_s_symbols_are_in_the_header_and_in_the_binding():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    for s in SYMS:
        assert s in ntm_amd._lib._SIGNATURES and re.search(r"\b%s\(" % s, header), s
        assert getattr(L, s).argtypes == ntm_amd._lib._SIGNATURES[s][1]
    assert len(ntm_amd._lib._SIGNATURES["ntm_adv_head_forward"][1]) == 10
    assert len(ntm_amd._lib._SIGNATURES["ntm_adv_head_backward"][1]) == 9
    assert L.ntm_abi_version() == 9 == ntm_amd._lib.ABI_VERSION and "#define NTM_ABI_VERSION 9" in header
    for name, value in (("NTM_ADV_HEAD_CRIT", ntm_amd._lib.ADV_HEAD_MODES["crit"]), ("NTM_ADV_HEAD_GEN", ntm_amd._lib.ADV_HEAD_MODES["gen"]),
                        ("NTM_ADV_HEAD_MAX_K", ntm_amd._lib.ADV_HEAD_MAX_K), ("NTM_ADV_HEAD_CHUNK", ntm_amd._lib.ADV_HEAD_CHUNK)):
        assert re.search(r"#define %s %d\b" % (name, value), header), name
    assert "advhead_kernels.hip" in open(os.path.join(ROOT, "neural-tape-modeling_amd", "csrc", "Makefile")).read()
    assert "adversarial" in ntm_amd.__all__ and "evaluation" in ntm_amd.__all__


def test_the_head_s_entry_points_check_their_arguments_before_any_launch():
    L = ntm_amd._lib.lib()
    one = ctypes.c_void_p(256)
    ptrs = lambda k: (ctypes.c_void_p * k)(*[256 + 64 * i for i in range(k)])      # noqa: E731
    el = ntm_amd._lib.i64_array

    def fwd(K=1, rows=2, n_fake=1, mode=0, outs=True, elems=(5,), ws=one, n_ws=1 << 20, loss=one):
        return L.ntm_adv_head_forward(ptrs(K) if outs else None, el(elems) if elems else None, K, rows, n_fake, mode, ws, n_ws, loss, None)

    def bwd(K=1, rows=2, n_fake=1, mode=0, elems=(5,), gout=one, grads=True, alias=False):
        return L.ntm_adv_head_backward(ptrs(K), el(elems), K, rows, n_fake, mode, gout, (ptrs(K) if alias else (ctypes.c_void_p * K)(*[4096] * K))
                                       if grads else None, None)

    for call, what in ((fwd, b"ntm_adv_head_forward"), (bwd, b"ntm_adv_head_backward")):
        for kw, msg in ((dict(mode=2), b"mode"), (dict(K=0, elems=()), b"[1, 8]"), (dict(K=9, elems=(5,) * 9), b"[1, 8]"),
                        (dict(rows=0), b"bad size"), (dict(n_fake=0), b"n_fake"), (dict(n_fake=2), b"n_fake"), (dict(elems=(0,)), b"bad size"),
                        (dict(rows=1 << 41, n_fake=1), b"2^40")):
            assert call(**kw) == -1, kw
            err = L.ntm_last_error()
            assert err.startswith(what) and msg in err, (kw, err)
    assert fwd(outs=False) == -1 and b"null pointer" in L.ntm_last_error()
    assert fwd(ws=None) == -1 and fwd(loss=None) == -1 and b"null pointer" in L.ntm_last_error()
    # the workspace: segments * chunks of the longest half -- 2 * ceil(3 * 5000 / 4096) = 8 doubles here
    assert fwd(rows=4, n_fake=1, elems=(5000,), n_ws=7) == -1 and b"workspace" in L.ntm_last_error()
    assert fwd(mode=1, rows=4, n_fake=0, elems=(5000,), n_ws=4) == -1 and b"workspace" in L.ntm_last_error()     # gen: 1 * ceil(20000 / 4096)
    assert bwd(gout=None) == -1 and bwd(grads=False) == -1 and b"null pointer" in L.ntm_last_error()
    assert bwd(alias=True) == -1 and b"alias" in L.ntm_last_error()


def test_the_float64_delay_entry_point_checks_its_arguments():
    header = open(os.path.join(ROOT, "include", "ntm.h")).read()
    L = ntm_amd._lib.lib()
    assert re.search(r"\bntm_delay_forward_f64\(", header) and "const double *d" in header
    assert L.ntm_delay_forward_f64.argtypes == ntm_amd._lib._SIGNATURES["ntm_delay_forward_f64"][1] == ntm_amd._lib._SIGNATURES["ntm_delay_forward"][1]
    one, two = ctypes.c_void_p(256), ctypes.c_void_p(4096)
    assert L.ntm_delay_forward_f64(one, one, two, -1, 4, one, 3, 0, None, None) == -1 and b"negative size" in L.ntm_last_error()
    assert L.ntm_delay_forward_f64(None, None, None, 0, 4, None, 3, 0, None, None) == 0
    assert L.ntm_delay_forward_f64(one, None, two, 2, 4, one, 3, 0, None, None) == -1 and b"null pointer" in L.ntm_last_error()
    assert L.ntm_delay_forward_f64(one, one, two, 2, 4, None, 3, 0, None, None) == -1 and b"null pointer" in L.ntm_last_error()
    assert L.ntm_delay_forward_f64(one, one, one, 2, 4, one, 3, 0, None, None) == -1 and b"alias" in L.ntm_last_error()
    assert L.ntm_delay_forward_f64(one, one, two, 65536, 4, one, 3, 0, None, None) == -1 and b"65535" in L.ntm_last_error()
    m = ntm_amd.DiffDelRNN(hidden_size=64, skip=False)
    with pytest.raises(RuntimeError, match="HIP device only"):
        m.forward_f64_delays(torch.zeros(2, 1, 8), torch.zeros(2, 1, 8, dtype=torch.float64))


def test_adv_head_fn_refuses_what_it_does_not_run():
    from ntm_amd.training import AdvHeadFn
    with pytest.raises(RuntimeError, match="HIP device only"):
        AdvHeadFn.apply("crit", 1, torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="'crit' and 'gen'"):
        AdvHeadFn.apply("hinge", 1, torch.zeros(2, 5))
    with pytest.raises(RuntimeError, match="outputs"):
        AdvHeadFn.apply("gen", 0)


def test_val_loss_supervised_keeps_the_reference_s_running_sums(monkeypatch):
    ev = ntm_amd.evaluation.val_loss_supervised(device="cpu")
    assert isinstance(ev, ntm_amd.ValLossSupervised) and ev.spec_scales == [2048, 1024, 512, 256, 128, 64]
    assert ev.losses == {k: 0 for k in KEYS} and ev.bst_losses == {k: [0, 1e9] for k in KEYS} and ev.iter_count == 0
    a = {k: float(i + 1) for i, k in enumerate(KEYS)}
    b = {k: 0.5 * (i + 1) for i, k in enumerate(KEYS)}
    feed = []
    monkeypatch.setattr(type(ev), "forward", lambda self, output, target: dict(feed.pop(0)))
    x = torch.zeros(2, 8)
    feed += [a, b]
    ev.add_loss(x, x)
    assert ev.losses == a and ev.iter_count == 1
    ev.add_loss(x, x)
    assert ev.losses == {k: a[k] + b[k] for k in KEYS} and ev.iter_count == 2
    ev.end_val(0)
    assert ev.iter_count == 0 and ev.bst_losses == {k: [0, (a[k] + b[k]) / 2] for k in KEYS}
    assert ev.losses == {k: a[k] + b[k] for k in KEYS}             # the sums stay readable until the next pass starts
    # a worse second epoch: the sums start again at the first add_loss, the best entries stay
    worse = {k: 10.0 * a[k] for k in KEYS}
    feed += [worse]
    ev.add_loss(x, x)
    assert ev.losses == worse and ev.iter_count == 1
    ev.end_val(1)
    assert ev.bst_losses == {k: [0, (a[k] + b[k]) / 2] for k in KEYS}
    # a better third one for a single key
    feed += [dict(worse, ESR=0.001)]
    ev.add_loss(x, x)
    ev.end_val(2)
    assert ev.bst_losses["ESR"] == [2, 0.001] and ev.bst_losses["MSE"] == [0, (a["MSE"] + b["MSE"]) / 2]
    assert ntm_amd.ValLossSupervised().spec_scales == (2048, 1024, 512, 256, 128, 64)      # the base class is as it was


def test_the_tool_s_command_line():
    t = tool()
    a = t.parser().parse_args([])
    assert a.load_config == '10' and a.DRY_RUN is False
    assert (a.AUDIO_PATH, a.DATASET_DIR, a.MODEL_PATH, a.EPOCHS, a.MAX_ITERS, a.FRACTION, a.SEED) == ("../audio/", None, None, 10000, None, 1.0, None)
    b = t.parser().parse_args(["-l", "3", "--DRY_RUN", "--EPOCHS", "2", "--MAX_ITERS", "1", "--FRACTION", "0.5", "--SEED", "7"])
    assert (b.load_config, b.DRY_RUN, b.EPOCHS, b.MAX_ITERS, b.FRACTION, b.SEED) == ("3", True, 2, 1, 0.5, 7)
    assert callable(t.main) and t.V_BS == 10
    with pytest.raises(ValueError, match="0, 1, 2, 3, 4, 5, 6, 7, 10"):
        t.main(["-l", "8", "--DRY_RUN"])
    # the collation of the three batch streams: the reference's (input, target, meta) with the trajectories in seconds
    items = [(torch.full((2, 6), float(i)), torch.full((2, 6), -float(i)), {"delay_trajectory": torch.full((6,), 0.01 * i), "input_name": "x"})
             for i in range(5)]
    got = list(t.batches(items, 2, [4, 0, 3, 1, 2]))
    assert [tuple(b[0].shape) for b in got] == [(2, 2, 6), (2, 2, 6), (1, 2, 6)] and got[0][0][:, 0, 0].tolist() == [4.0, 0.0]
    assert got[1][2]["delay_trajectory"].shape == (2, 6) and got[1][1][:, 0, 0].tolist() == [-3.0, -1.0]
    assert len(list(t.batches(items, 2, [4, 0, 3, 1, 2], max_iters=1))) == 1


def test_dry_run_writes_no_file(tmp_path):
    """The tool stops early here -- at "HIP device only" without a device, at the missing dataset directory with one -- and both
    come after the point where the reference creates its checkpoint directory (code/train-adversarial.py:91-92): with --DRY_RUN
    nothing has been written by then, without it the directory."""
    t = tool()
    dry, wet = tmp_path / "dry", tmp_path / "wet"
    stop = (OSError, ValueError, AssertionError) if torch.cuda.is_available() else RuntimeError
    with pytest.raises(stop, match=None if torch.cuda.is_available() else "HIP device only"):
        t.main(["--DRY_RUN", "--MODEL_PATH", str(dry), "--DATASET_DIR", str(tmp_path / "none")])
    assert not dry.exists() and list(tmp_path.iterdir()) == []
    with pytest.raises(stop):
        t.main(["--MODEL_PATH", str(wet), "--DATASET_DIR", str(tmp_path / "none")])
    assert [p.name for p in wet.iterdir()] == ["UnpairedTraining_10"] and list((wet / "UnpairedTraining_10").iterdir()) == []


def test_a_trainer_on_cpu_parameters_is_refused():
    import contextlib
    import io
    gen = ntm_amd.DiffDelRNN(hidden_size=64, skip=False)
    with contextlib.redirect_stdout(io.StringIO()):
        crit = ntm_amd.critics.DilatedConvDisc(layers=6, conv_channels=16, test_in_len=1024)
    optG = torch.optim.Adam(gen.parameters(), lr=1e-4, betas=(0.5, 0.9))
    optC = torch.optim.Adam(crit.parameters(), lr=1e-4, betas=(0.5, 0.9))
    with pytest.raises(RuntimeError, match="HIP device only"):
        ntm_amd.adversarial.Trainer(gen, crit, optG, optC, 1024, 44100, 400.25 / 44100, 700.75 / 44100)
    assert not any(p.requires_grad for p in gen.parameters())          # refused before anything was touched


def test_golden_g28_is_what_its_maker_says():
    g = np.load(os.path.join(GOLDEN, "g28_adversarial.npz"))
    seed, iters, B, fs, win, nwin, t_val, knot = (int(v) for v in g["meta"])
    assert (iters, B, fs, win, nwin, t_val) == (2, 2, 44100, 1024, 2, 3000)
    T = 1024 + nwin * win
    assert g["x_gen"].shape == g["x_crit"].shape == g["t_real"].shape == (iters, B, 1, T) and g["x_gen"].dtype == np.float32
    assert g["traj_knots"].shape == (iters, 2, B, T // knot + 1) and g["traj_knots"].dtype == np.float64
    d_min, d_max = float(g["d_min_s"]), float(g["d_max_s"])
    assert d_min <= g["traj_knots"].min() and g["traj_knots"].max() <= d_max
    assert max(int((d_max * fs + 1) - (d_min * fs - 1)) + 2, 1024) == 1024 and int(d_min * fs - 1) - 1 == 398
    assert g["ref64__crit_losses"].shape == g["ref64__gen_losses"].shape == (iters * nwin,)
    for kind in ("crit_loss", "gen_loss", "val", "crit_grad", "gen_grad"):
        assert 0 < float(g[f"e32__{kind}"]) < 1e-2, kind            # four times it stays far from passing a zero tensor
    assert os.path.getsize(os.path.join(GOLDEN, "g28_adversarial.npz")) < 700 * 1024
