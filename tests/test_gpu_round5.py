"""Round 5: ANY hidden size (the reference's `--HIDDEN_SIZE` is a free integer, code/train.py:50, code/model.py:22,44-45) against
goldens made by the reference itself (g21, tools/make_goldens_anyh.py) and the oracle; the evaluation CLI's loss cache
(tools/test_model.py) with directory-path weights and changed arguments; the DCPreESR sums out of the recurrent launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
from helpers import ROOT, bench_record, load

pytestmark = pytest.mark.gpu

TOL = 1e-5          # north_star: |hip - PyTorch-CPU fp32| < 1e-5


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _from_golden(ntm, g, prefix, H, cls, **kw):
    m = cls(1, H, 1, **kw)
    m.load_state_dict({k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)})   # reference format, strict
    return m.to("cuda").eval()


# ----------------------------------------------------------------------------- any hidden size
@pytest.mark.parametrize("H", [5, 24, 48, 96, 200])
def test_g21_any_hidden_size_vs_reference(ntm, H):
    """H = 5 / 24 / 48: the small kernel zero-padded to 8 / 32 / 64; H = 96: the register-resident wide kernel; H = 200:
    the plain one.  predict per stream == the reference's B = 1 predict, batched forward with state carry, chunked ==
    one-shot bit for bit."""
    g = load("g21_any_hidden_size.npz")
    m = _from_golden(ntm, g, f"sd_{H}_", H, ntm.RNN)
    assert m.hidden_size == H and tuple(m.GRU.weight_hh_l0.shape) == (3 * H, H)
    x = dev(g[f"x_{H}"])
    y = m.predict(x)
    assert np.abs(y.cpu().numpy() - g[f"y_{H}_predict"]).max() < TOL
    for b in range(3):
        assert np.abs(m.predict(x[b:b + 1]).cpu().numpy() - g[f"y_{H}_predict"][b:b + 1]).max() < TOL
    m.initialize_hidden()
    y0, y1 = m(x[:, :, :700]), m(x[:, :, 700:])
    assert np.abs(torch.cat([y0, y1], 2).cpu().numpy() - g[f"y_{H}_carry"]).max() < TOL
    assert np.abs(m.hidden.cpu().numpy() - g[f"h_{H}_carry"]).max() < TOL
    assert torch.equal(m.predict(x, segment_length=2048), y) and torch.equal(m.predict(x, segment_length=333), y)
    for variant in ("lat", "valu"):                     # the variants the small sizes accept all resolve to the same kernel
        m.kernel_variant = variant
        assert torch.equal(m.predict(x), y)
    m.kernel_variant = "mfma2"
    with pytest.raises(ntm.NtmError):                   # the matrix-pipe variants exist for H = 64 only
        m.predict(x)


@pytest.mark.parametrize("H", [1, 3, 5, 9, 24, 33, 48, 63, 65, 96, 127, 128, 129, 200, 300, 1024])
@pytest.mark.parametrize("B,T", [(1, 1), (7, 63), (9, 64), (5, 65), (70, 129), (131, 400)])
def test_any_hidden_size_ragged_vs_oracle(ntm, H, B, T):
    """Ragged batches (B not a multiple of the streams of a wavefront, T around the 64-sample tile), a non-zero initial
    state, every boundary of the kernel choice (H = 63 | 65, 128 | 129)."""
    rng = np.random.default_rng(1000 * H + B + T)
    torch.manual_seed(H)
    m = ntm.RNN(1, H, 1).to("cuda").eval()
    w = oracle.Weights.from_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items()})
    x = rng.uniform(-0.7, 0.7, (B, T)).astype(np.float32)
    h0 = rng.uniform(-0.9, 0.9, (B, H)).astype(np.float32)
    m.hidden = dev(h0).view(1, B, H)
    y = m(dev(x).unsqueeze(1))
    yo, ho = oracle.gru_forward(w, x, h0, threads=8)
    assert np.abs(y[:, 0].cpu().numpy() - yo).max() < TOL and np.abs(m.hidden[0].cpu().numpy() - ho).max() < TOL


def test_g21_diffdel_hidden_24(ntm):
    """DiffDelRNN at a hidden size without a kernel of its own: GRU launch (padded kernel) + the streaming delay pass."""
    g = load("g21_any_hidden_size.npz")
    md = int(g["dd_max_delay"])
    m = _from_golden(ntm, g, "dd_sd_", 24, ntm.DiffDelRNN, max_delay=md)
    y, pre = m.predict(dev(g["dd_x"]), dev(g["dd_d"]))
    assert np.abs(pre.cpu().numpy() - g["dd_pre_d"]).max() < TOL and np.abs(y.cpu().numpy() - g["dd_y"]).max() < TOL
    assert np.abs(m.diffdel.buffer.cpu().numpy() - g["dd_buffer"]).max() < TOL
    assert np.abs(m.hidden.cpu().numpy() - g["dd_hidden"]).max() < TOL
    # batched, against the oracle
    rng = np.random.default_rng(24)
    B, T = 37, 900
    x = rng.uniform(-0.6, 0.6, (B, T)).astype(np.float32)
    d = (150.0 + 120.0 * np.sin(np.arange(T) / 41.0 + rng.uniform(0, 6, (B, 1)))).astype(np.float32)
    w = oracle.Weights.from_state_dict({k[len("dd_sd_"):]: g[k] for k in g.files if k.startswith("dd_sd_")})
    yb, pb = m.predict(dev(x).unsqueeze(1), dev(d).unsqueeze(1))
    yo, po, _, _ = oracle.diffdel_predict(w, x, d, md)
    assert np.abs(pb[:, 0].cpu().numpy() - po).max() < TOL and np.abs(yb[:, 0].cpu().numpy() - yo).max() < TOL
    m.delay_mode = "fused"
    with pytest.raises(ntm.NtmError):                   # the fused step is the H = 64 kernel
        m.predict(dev(x).unsqueeze(1), dev(d).unsqueeze(1))


@pytest.mark.parametrize("H", [24, 96])
def test_forward_esr_any_hidden_size(ntm, H):
    """ntm_gru_forward_esr for a size without the matrix-pipe kernel: forward launch + the streaming ESR pass."""
    rng = np.random.default_rng(H)
    torch.manual_seed(50 + H)
    m = ntm.RNN(1, H, 1).to("cuda").eval()
    w = oracle.Weights.from_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items()})
    B, T, skip = 1100, 300, 64
    x = rng.uniform(-0.6, 0.6, (B, T)).astype(np.float32)
    t = (0.4 * x + 0.01).astype(np.float32)
    y, s = m.predict_esr(dev(x).unsqueeze(1), dev(t).unsqueeze(1), skip=skip)
    rows = [0, 555, B - 1]
    yo, _ = oracle.gru_predict(w, x[rows])
    assert np.abs(y[rows, 0].cpu().numpy() - yo).max() < TOL
    so = oracle.esr_sums(y[rows, 0].cpu().numpy(), t[rows], skip)
    assert np.abs(s[rows].cpu().numpy() / so - 1).max() < 1e-9


def test_any_hidden_size_through_the_c_abi_strided(ntm):
    """Row strides (the ABI takes them) and NULL h_state through ntm_gru_forward at H = 48 and 96."""
    L = ntm._lib.lib()
    from ntm_amd._lib import ptr
    for H in (48, 96):
        torch.manual_seed(H)
        m = ntm.RNN(1, H, 1).to("cuda").eval()
        w = oracle.Weights.from_state_dict({k: v.cpu().numpy() for k, v in m.state_dict().items()})
        rng = np.random.default_rng(H)
        B, T, XS, YS = 6, 150, 170, 190
        xs = torch.zeros(B, XS, device="cuda")
        xs[:, :T] = dev(rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32))
        ys = torch.full((B, YS), 7.0, device="cuda")
        g, o = m.GRU, m.output
        rc = L.ntm_gru_forward(ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0), ptr(o.weight), ptr(o.bias),
                               H, ptr(xs), ptr(ys), B, T, XS, YS, None, ntm._lib.current_stream())
        assert rc == 0, L.ntm_last_error()
        yo, _ = oracle.gru_forward(w, xs[:, :T].cpu().numpy())
        assert np.abs(ys[:, :T].cpu().numpy() - yo).max() < TOL and bool((ys[:, T:] == 7.0).all())


# ----------------------------------------------------------------------------- the CLI's loss cache
def test_cli_loss_cache_with_directory_weights_and_changed_arguments(tmp_path, monkeypatch, capsys):
    """A `--WEIGHTS` entry that is a directory path (slashes) must not break the cache write after the whole evaluation; a
    second run with the same arguments loads the cache, one with another --SEGMENT_LENGTH or --KERNEL recomputes, --NO_CACHE
    neither reads nor writes; a HS[24] checkpoint in the reference's best.pth format runs through the whole command."""
    from test_cli import _wow_dataset, cli_module
    cli = cli_module("ntm_cli_r5")
    g, fs, N, audio, tgt_audio = _wow_dataset(tmp_path, "Wow")
    monkeypatch.chdir(tmp_path)
    name = "GRU-HS[24]-L[ESR]-DS[Wow]_1"
    wdir = tmp_path / "some" / "where" / name
    wdir.mkdir(parents=True)
    torch.manual_seed(24)
    ref = torch.nn.GRU(1, 24, batch_first=True)
    lin = torch.nn.Linear(24, 1)
    sd = {"GRU." + k: v.detach().clone() for k, v in ref.state_dict().items()}
    sd.update({"output." + k: v.detach().clone() for k, v in lin.state_dict().items()})
    torch.save(sd, str(wdir / "best.pth"))
    L = 12000
    argv = ["--MODEL", "GRU", "--WEIGHTS", str(wdir), "--DATASET_DIR", str(tmp_path / "Wow"), "--SUBSET", "Test", "--NO_SHUFFLE",
            "--SEGMENT_LENGTH", str(L), "--COMPUTE_LOSS", "--NO_EXAMPLE", "--TEMP_PATH", str(tmp_path / "tmp")]
    got = cli.main(argv)
    out = capsys.readouterr().out
    assert "Starting analysis" in out and "Stats:" in out and "cache not written" not in out
    cache = list((tmp_path / "tmp" / "loss" / "Wow" / "Test").glob("*.npy"))
    assert len(cache) == 1 and name in cache[0].name and os.sep not in cache[0].name
    # the .npy holds exactly what upstream's does -- a plain {loss: float} dict its stats loop can format
    # (code/test-model.py:399-403,414-415) -- and the argument record sits in a side-car; an upstream-written cache (no
    # side-car) is recomputed, not trusted
    import json
    blob = np.load(str(cache[0]), allow_pickle=True).item()
    assert set(blob) == set(got) and all(isinstance(v, float) and "{:.6f}".format(v) for v in blob.values())
    rec = json.load(open(str(cache[0])[:-4] + ".key.json"))
    assert rec["segments"] == N // 12000 and rec["key"]["segment_length"] == 12000 and rec["key"]["kernel"] == "auto"
    # the numbers: the oracle on the same segments with the same checkpoint
    T = g["T1"]
    init = 1 << (int(T.max() * fs) - 1).bit_length()
    nseg = N // L
    X = np.stack([audio[k * L:(k + 1) * L] for k in range(nseg)])
    Tg = np.stack([tgt_audio[k * L:(k + 1) * L] for k in range(nseg)])
    w = oracle.Weights.from_state_dict({k: v.numpy() for k, v in sd.items()})
    want = float(np.mean(oracle.esr_per_segment(oracle.gru_predict(w, X)[0], Tg, init)))
    assert abs(got["ESR"] - want) < 1e-3 * want
    assert cli.main(argv) == got and "Loading pre-computed!" in capsys.readouterr().out
    other = cli.main(argv[:argv.index("--SEGMENT_LENGTH") + 1] + ["9000"] + argv[argv.index("--SEGMENT_LENGTH") + 2:])
    out = capsys.readouterr().out
    assert "recomputing" in out and "Starting analysis" in out and other["ESR"] != got["ESR"]
    assert cli.main(argv) != other and "recomputing" in capsys.readouterr().out           # ... and back: the file holds the 9000 run now
    os.remove(str(cache[0])[:-4] + ".key.json")                  # what an upstream-written cache looks like
    assert cli.main(argv) == got and "no argument record" in capsys.readouterr().out
    stamp = cache[0].stat().st_mtime_ns
    assert cli.main(argv + ["--NO_CACHE"]) == got
    out = capsys.readouterr().out
    assert "Starting analysis" in out and cache[0].stat().st_mtime_ns == stamp


# ----------------------------------------------------------------------------- chunked TCN call: asynchronous, repeatable, capturable
def test_chunked_tcn_call_returns_before_its_work_and_can_be_captured(ntm):
    """the two lane streams of a chunked ntm_tcn_forward were created and destroyed per call (a destroy
    may wait for the queue).  They are a per-device pool now: the host returns while the device is still busy (host time of
    the call well under the event-timed duration), repeated calls give the same bits, and the fork / join on pooled streams
    is capturable into a HIP graph whose replay gives those bits again."""
    import time
    L = ntm._lib.lib()
    B, T = 8, 1 << 23
    assert L.ntm_tcn_chunk_streams(B, T, 32) == 1          # 8 chunks of one stream on two lanes
    tcn = ntm.TCN().to("cuda")
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.rand(B, 1, T, generator=g, device="cuda") - 0.5
    y0 = tcn(x)                                             # builds the pool, sizes the scratch
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    host, devms = [], []
    for _ in range(3):
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        y = tcn(x)
        host.append(1e3 * (time.perf_counter() - t0))
        e1.record()
        torch.cuda.synchronize()
        devms.append(e0.elapsed_time(e1))
        assert torch.equal(y, y0)
    assert min(host) < 0.5 * min(devms), (host, devms)
    # the same call under stream capture (torch allocates y from the graph's private pool): a captured call keeps to the
    # caller's stream (the pooled lanes are shared, a lane forked into one capture would pull a concurrent
    # call of another thread into it), so an un-captured call on another stream WHILE the capture is open must go through
    s = torch.cuda.Stream()
    other = torch.cuda.Stream()
    L_ = ntm._lib
    y_other = torch.empty_like(x)                           # everything the un-captured call needs exists before the capture opens
    scratch = torch.empty(int(L.ntm_tcn_scratch_floats(B, T, 32)), device="cuda")
    packed = tcn.packed_params()
    dil = (ctypes.c_int * len(tcn.dilations))(*tcn.dilations)
    torch.cuda.synchronize()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s, capture_error_mode="relaxed"):
            yg = tcn(x)
            rc = L.ntm_tcn_forward(L_.ptr(packed), len(tcn.dilations), 32, 13, dil, L_.ptr(x), L_.ptr(y_other), B, T,
                                   L_.ptr(scratch), ctypes.c_void_p(other.cuda_stream))       # not part of the capture: on the lanes, now
            assert rc == 0, L.ntm_last_error()
    other.synchronize()
    assert torch.equal(y_other, y0)
    torch.cuda.current_stream().wait_stream(s)
    yg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, y0)


# ----------------------------------------------------------------------------- other_workloads.cli of the bench line
def test_bench_cli_workload_stage_times_and_cpu_port():
    """bench.py's `other_workloads.cli` (the reference's evaluation command end to end, scripts/test-model-loss.sh:57-63) at a
    small shape: two 1-second segments, so that the command's losses can be compared with the torch-CPU port of the same
    command on the same two segments; every stage carries a time, the GPU-busy fractions are fractions."""
    import sys
    sys.path.insert(0, ROOT)
    import bench
    r = bench.cli_workload(torch.device("cuda", 0), True, n_seg=2, L=44100)
    assert r["unit"] == "samples/s" and r["value"] > 0 and abs(r["value"] - 2 * 44100 / r["command_s"]) < 1e-6 * r["value"]
    assert r["dataset_resident_on_device"] is True
    assert set(r["stages_ms"]) == {"decode (WAV -> device, side-car)", "gather (device to device)", "predict", "apply_delay", "ESR", "DCPreESR", "MultiSTFT"}
    assert all(v > 0 for v in r["stages_ms"].values()) and r["bound_by"] in r["stages_ms"]
    assert 0 < r["gpu_busy_fraction_of_command"] <= r["gpu_busy_fraction_of_loss_loop"] <= 1.0
    cpu = r["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and set(cpu["stages_s"]) == {"predict_s", "apply_delay_s", "ESR_s", "DCPreESR_s", "MultiSTFT_s"}
    for k in ("ESR", "DCPreESR", "MultiSTFT"):           # same command, same two segments: the CPU port's losses
        assert abs(r["losses"][k] / cpu["losses"][k] - 1) < 2e-3, (k, r["losses"], cpu["losses"])
    assert "scripts/test-model-loss.sh" in r["reference_command"] and not os.path.exists("/tmp/ntm_cli_leftover")


# ----------------------------------------------------------------------------- DCPreESR sums out of the recurrent launch
W_G = "GRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE]_BEST"


@pytest.mark.parametrize("B,T,skip", [(1040, 64, 0), (1040, 300, 64), (1040, 4136, 1024), (1040, 1000, 4), (1300, 777, 128),
                                      (4112, 500, 64), (4200, 700, 256), (1040, 300, 2), (700, 300, 64), (1040, 5, 0), (1040, 129, 128)])
def test_forward_losses_esr_and_dcpre_in_one_launch(ntm, B, T, skip):
    """RNN.predict_losses (ntm_gru_forward_losses): y bit-identical to predict(), the ESR sums bit-identical to
    predict_esr's, the DCPreESR sums against the streaming kernel on the same output (fp32 filter in another evaluation
    order: 2e-6 rel) and against the oracle's sequential recursion (2e-5 rel, the streaming kernel's own bar).  Shapes: one /
    several / ragged 64-sample tiles, skip inside a tile and beyond the first tile, 4112 = whole device rounds + a remainder
    on the low-latency kernel, 4200 > 4096 (three workgroups per CU, YPN = 4), skip = 2 and B = 700 (no fused launch: forward
    + the two streaming passes)."""
    rng = np.random.default_rng(B + T + skip)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    t = (0.6 * np.tanh(1.7 * x) + 0.05 + 0.01 * rng.standard_normal((B, T))).astype(np.float32)     # a DC offset for the blocker
    xd, td = dev(x).unsqueeze(1), dev(t).unsqueeze(1)
    m = ntm.harness.build_model(W_G)
    y, s, d = m.predict_losses(xd, td, skip=skip)
    h = m.hidden.clone()
    y0 = m.predict(xd)
    assert torch.equal(y, y0) and torch.equal(m.hidden, h)
    y1, s1 = m.predict_esr(xd, td, skip=skip)
    assert torch.equal(y1, y0) and torch.equal(s1, s)
    d_stream = ntm.esr_dcpre_sums(y0, td, skip).cpu().numpy()
    got = d.cpu().numpy()
    assert np.isfinite(got).all()
    scale = np.maximum(np.abs(d_stream), 1e-30)
    assert (np.abs(got - d_stream) / scale).max() < 2e-6 or T - skip <= 1, (np.abs(got - d_stream) / scale).max()
    rows = [0, 15, 16, B // 2, B - 1]
    want = oracle.esr_dcpre_sums(y0[rows, 0].cpu().numpy(), t[rows], skip)
    assert np.allclose(got[rows], want, rtol=2e-5, atol=1e-12)
    # another pole, and R = 0 (a plain first difference)
    for R in (0.9, 0.0):
        _, _, dr = m.predict_losses(xd, td, skip=skip, R=R)
        assert np.allclose(dr[rows].cpu().numpy(), oracle.esr_dcpre_sums(y0[rows, 0].cpu().numpy(), t[rows], skip, R), rtol=2e-5, atol=1e-12)


def test_forward_losses_on_a_ten_second_segment_and_through_the_c_abi(ntm):
    """441 000 samples (6890 whole tiles + 40 samples: the ragged last tile), INIT_LEN 2048 as the toy data gives; then the C
    entry point's argument checks (nothing enqueued on NTM_EINVAL)."""
    rng = np.random.default_rng(9)
    B, T, skip = 1040, 441000, 2048
    x1 = (0.4 * np.sin(np.arange(T) * 0.03) * (0.6 + 0.4 * np.sin(np.arange(T) * 1e-4)) + 0.02 * rng.standard_normal(T)).astype(np.float32)
    t1 = (0.5 * np.tanh(2.0 * x1) + 0.02).astype(np.float32)
    xd = dev(np.broadcast_to(x1, (B, T)).copy()).unsqueeze(1)
    td = dev(np.broadcast_to(t1, (B, T)).copy()).unsqueeze(1)
    m = ntm.harness.build_model(W_G)
    y, s, d = m.predict_losses(xd, td, skip=skip)
    assert torch.equal(d[0], d[519]) and torch.equal(d[0], d[B - 1]) and torch.equal(s[0], s[B - 1])
    want = oracle.esr_dcpre_sums(y[:1, 0].cpu().numpy(), t1[None], skip)
    assert np.allclose(d[:1].cpu().numpy(), want, rtol=2e-5)
    L = ntm._lib.lib()
    one, two, three = (ctypes_ptr(v) for v in (16, 32, 48))
    assert L.ntm_gru_forward_losses(one, one, one, one, one, None, 64, one, two, 4, 100, 100, 100, None, three, 0, one, 0.995, None, None) == -1
    assert L.ntm_gru_forward_losses(one, one, one, one, one, None, 64, one, two, 4, 100, 100, 100, None, three, 0, one, 1.5, two, None) == -1
    assert b"R must be in [0,1)" in L.ntm_last_error()
    assert L.ntm_gru_forward_losses(one, one, one, one, one, None, 64, one, two, 4, 100, 100, 100, None, three, 0, one, 0.995, one, None) == -1
    assert b"distinct" in L.ntm_last_error()
    assert L.ntm_gru_forward_losses(one, one, one, one, one, None, 64, one, two, 0, 100, 100, 100, None, three, 0, one, 0.995, two, None) == 0


def ctypes_ptr(v):
    import ctypes
    return ctypes.c_void_p(v)


def test_cli_fused_losses_path_matches_the_separate_passes(tmp_path, monkeypatch):
    """tools/test_model.py with --STREAM_CHUNK 0 on a plain GRU evaluation issues predict + ESR + DCPreESR as one call
    (RNN.predict_losses); same losses as the default streamed pipeline with its separate passes."""
    from test_cli import _wow_dataset, cli_module
    cli = cli_module("ntm_cli_r5b")
    _wow_dataset(tmp_path, "Wow")
    monkeypatch.chdir(tmp_path)
    argv = ["--MODEL", "GRU", "--WEIGHTS", W_G, "--DATASET_DIR", str(tmp_path / "Wow"), "--SUBSET", "Test", "--NO_SHUFFLE",
            "--SEGMENT_LENGTH", "12000", "--COMPUTE_LOSS", "--NO_EXAMPLE", "--NO_CACHE"]
    prof_a, prof_b = {}, {}
    a = cli.main(argv, profile=prof_a)
    b = cli.main(argv + ["--STREAM_CHUNK", "0"], profile=prof_b)
    assert "predict_streamed_ms" in prof_a and "ESR_ms" in prof_a and "DCPreESR_ms" in prof_a
    assert "predict+ESR+DCPreESR_ms" in prof_b and "ESR_ms" not in prof_b and "DCPreESR_ms" not in prof_b and prof_b["h2d_ms"] > 0
    assert abs(a["ESR"] / b["ESR"] - 1) < 1e-9 and abs(a["DCPreESR"] / b["DCPreESR"] - 1) < 1e-5 and abs(a["MultiSTFT"] / b["MultiSTFT"] - 1) < 1e-9


# ----------------------------------------------------------------------------- the device-resident decode
@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.uint8, np.float32, np.float64])
@pytest.mark.parametrize("channels", [1, 2])
def test_read_wav_device_equals_the_host_decode(tmp_path, monkeypatch, dtype, channels):
    """feeder.read_wav_device (mapped file -> pinned staging chunks -> H2D -> de-interleave / convert / scale on the device)
    gives the bits of the host decode for every PCM / float format, mono and stereo, across staging-chunk boundaries (the
    chunk is shrunk to 4 kB here: 40 chunks, both staging pairs reused many times)."""
    from scipy.io import wavfile
    from ntm_amd import feeder as F
    monkeypatch.setattr(F, "_STAGE_BYTES", 4096)
    F._stage.clear()
    rng = np.random.default_rng(11)
    N = 20011
    if dtype == np.uint8:
        a = rng.integers(0, 256, (N, channels)).astype(dtype)
    elif dtype in (np.int16, np.int32):
        info = np.iinfo(dtype)
        a = rng.integers(info.min, info.max, (N, channels), endpoint=True).astype(dtype)
        a[0], a[1] = info.min, info.max
    else:
        a = rng.uniform(-1, 1, (N, channels)).astype(dtype)
    path = str(tmp_path / "f.wav")
    wavfile.write(path, 32000, a[:, 0] if channels == 1 else a)
    want, fs0 = F.read_wav(path)
    got, fs1 = F.read_wav_device(path)
    F._stage.clear()                                              # (the 4 kB buffers must not outlive the test)
    assert fs0 == fs1 == 32000 and got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (channels, N) and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy(), want)


def test_resident_and_pinned_host_layouts_are_the_same_dataset(tmp_path):
    """SegmentFeeder(resident=True) (the default on a HIP device: the decode is the H2D copy, the set lives in HBM) against
    resident=False (pinned host, H2D per batch): items, statistics, batches and shards bit for bit -- int16 mono files of
    uneven length, and a stereo float pair with a trajectory side-car."""
    from scipy.io import wavfile
    from ntm_amd.feeder import SegmentFeeder, write_sidecar
    rng = np.random.default_rng(5)
    d = tmp_path / "Set" / "Val"
    d.mkdir(parents=True)
    L = 2500
    for i, n in enumerate((3 * L + 11, L, 2 * L + 999)):
        x = (rng.uniform(-0.5, 0.5, n) * 32767).astype(np.int16)
        wavfile.write(str(d / f"input_{i}_.wav"), 44100, x)
        wavfile.write(str(d / f"target_{i}_.wav"), 44100, (0.25 * x).astype(np.int16))
    N = 4 * L + 5
    a = rng.uniform(-0.4, 0.4, (N, 2)).astype(np.float32)
    wavfile.write(str(d / "input_7_.wav"), 44100, a)
    wavfile.write(str(d / "target_7_.wav"), 44100, (0.5 * a).astype(np.float32))
    traj = 0.003 + 0.001 * np.sin(np.arange(N) / 300.0)
    peaks = np.arange(100, N - 100, 441)
    meta = {"reconstruction_percentage": 0.0, "wiggle_percentage": 0.0}
    write_sidecar(str(d / "trajectory_7_.npy"), peaks, peaks + 130, traj, meta, meta)
    fa = SegmentFeeder(str(tmp_path / "Set"), subset="val", length=L, resident=False)
    fb = SegmentFeeder(str(tmp_path / "Set"), subset="val", length=L)
    assert fa.resident is False and fb.resident is True and len(fa) == len(fb) == 10
    assert (fa.mean_delay, fa.max_delay, fa.min_delay, fa.fs, fa.minutes) == (fb.mean_delay, fb.max_delay, fb.min_delay, fb.fs, fb.minutes)
    for i in range(len(fa)):
        ia, ib = fa[i], fb[i]
        assert not ib[0].is_cuda and torch.equal(ia[0], ib[0]) and torch.equal(ia[1], ib[1]) and ia[2]["input_name"] == ib[2]["input_name"]
        if "delay_trajectory" in ia[2]:
            assert torch.equal(ia[2]["delay_trajectory"], ib[2]["delay_trajectory"])
    for bs in (4, 10):
        for rank, world in ((0, 1), (1, 3)):
            for (xa, ta, da, ma), (xb, tb, db, mb) in zip(fa.batches(bs, "cuda", rank, world), fb.batches(bs, "cuda", rank, world)):
                assert torch.equal(xa, xb) and torch.equal(ta, tb) and ma == mb
                assert (da is None) == (db is None) and (da is None or torch.equal(da, db))


# ----------------------------------------------------------------------------- the N-rank line under the driver's launcher
def test_bench_under_torch_distributed_run_two_ranks():
    """The driver starts N > 1 as `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N ...`: the launcher's environment (TORCHELASTIC_*, GROUP_RANK, LOCAL_WORLD_SIZE,
    OMP_NUM_THREADS=1) must not leak into rank 0's post-teardown legs -- the live counter passes are single-GPU child
    commands, the CPU baseline uses the host's cores.  Two ranks share this box's GPU over gloo, 1040 x 65 536 per rank."""
    import json
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["NTM_DIST_BACKEND"] = "gloo"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--batch", "1040", "--full", "--cpu-sample", "small", "--no-extra"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line, d = bench_record(r.stdout)            # the N-rank compact line: < 4 KB, parseable, roofline + cpu_baseline on it
    assert line["n_gpus"] == 2 and line["cpu_baseline"]["value"] > 0 and line["roofline"]["aggregate"]["n_gpus"] == 2
    assert line["roofline"]["traffic_live"] is True and 1.0 <= line["roofline"]["traffic_ratio"] < 1.02
    assert line["checks"]["streams_vs_oracle_max_abs"] < TOL and line["checks"]["esr_sums_max_rel"] < 1e-9
    assert d["n_gpus"] == 2 and d["ranks"] == 2 and d["backend"] == "gloo" and d["config"]["segments_total"] == 2080
    assert d["metric"] == "audio samples/sec (44.1 kHz) GRU-HS[64], batch=1040x65536 per GPU, 2 GPU (weak scaling, 2080 segments)"
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["cores"] == min(32, len(os.sched_getaffinity(0)))
    assert d["checks"]["streams_vs_oracle"]["max_abs"] < TOL and d["checks"]["esr_sums_vs_oracle"]["max_rel"] < 1e-9
    rf = d["roofline"]
    assert rf["segments_in_launch"] == 1040 and rf["traffic"] is not None and "measured in this run" in rf["traffic_source"], rf["traffic_source"]
    assert 1.0 <= rf["traffic"] / rf["algorithmic_bytes"] < 1.02
    assert rf["aggregate"]["n_gpus"] == 2 and len(rf["aggregate"]["kernel_ms_by_rank"]) == 2 and "other_workloads" not in d


# ----------------------------------------------------------------------------- configs[1] / [2]: EVERY stream of the full batch
FULL = pytest.mark.skipif(os.environ.get("NTM_SKIP_FULL") == "1", reason="full 4096x65536 passes skipped on request")
W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"


def _record_full(name, **row):
    import json
    path = os.path.join(ROOT, "gpurun_out", "r06_full_batch_parity.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    lib = os.path.basename(os.environ.get("NTM_LIB_PATH") or "libntm.so")       # (an A/B build reached through NTM_LIB_PATH is named in the record)
    with open(path, "a") as f:
        f.write(json.dumps(dict(config=name, library=lib, **row)) + "\n")


def _margin(hip, or32, f64):
    """Per stream: |hip - f64|, |oracle32 - f64| (the fp32 restatement's OWN rounding error on that stream) and their ratio --
    how much of the 1e-5 bar the device's arithmetic uses, separated from what any fp32 evaluation of the recurrence uses.
    -> dict of the distribution over the streams (worst / p99 / median each, the worst stream's numbers, the ratio's)."""
    dh = np.abs(hip - f64).max(axis=1)
    do = np.abs(or32 - f64).max(axis=1)
    ratio = dh / np.maximum(do, 1e-12)
    q = lambda v: {"worst": float(v.max()), "p99": float(np.quantile(v, 0.99)), "median": float(np.median(v))}      # noqa: E731
    i = int(dh.argmax())
    return {"hip_vs_f64": q(dh), "oracle32_vs_f64": q(do), "ratio_per_stream": q(ratio), "ratio_of_worsts": float(dh.max() / do.max()),
            "worst_stream": {"stream": i, "hip_vs_f64": float(dh[i]), "oracle32_vs_f64": float(do[i])}}


@FULL
def test_full_size_cfg2_every_stream_against_the_oracle(ntm):
    """BASELINE configs[1] at full size, ALL 4096 streams x 65 536 samples against the C oracle (rounds 2-4 checked 36
    scattered streams: the torch-CPU reference takes half an hour for the batch, the OpenMP oracle -- itself pinned to the
    reference by goldens g1 / g2 / g6 / g19 / g20 -- about 20 s on the box's cores).  Output and carried state of every
    stream inside 1e-5.  Round 6: the oracle's fp64 mode (pinned to torch's double modules by g20) separates the device's
    rounding from the fp32 oracle's own: per stream |hip - f64| and |oracle32 - f64|; the distributions go into
    gpurun_out/r06_full_batch_parity.jsonl (round 6 ran it once more with an A/B build of the other tanh form through
    NTM_LIB_PATH: profiles/r06_b_full_batch_parity.jsonl; not adopted, the build is retired)."""
    import sys
    import time
    from helpers import oracle_weights
    sys.path.insert(0, ROOT)
    import bench
    B, T = 4096, 65536
    threads = max(1, min(32, len(os.sched_getaffinity(0))))      # (256 threads on the box were 2.7 x SLOWER than 32)
    x = bench.synth_input(B, T, torch.device("cuda", 0), seed=1234)
    m = ntm.harness.build_model(W_G)
    y = m.predict(x).cpu().numpy()[:, 0]
    h = m.hidden[0].cpu().numpy()
    # the opt-in split engines on the same batch (round 6: the table the bf16x3 engine is judged by)
    y_eng = {}
    for eng in ("f16x3", "bf16x3"):
        m.kernel_variant = eng
        y_eng[eng] = m.predict(x).cpu().numpy()[:, 0]
    m.kernel_variant = "auto"
    xs = x[:, 0].cpu().numpy()
    del x
    t0 = time.perf_counter()
    yo, ho = oracle.gru_predict(oracle_weights(W_G), xs, threads=threads)
    dt = time.perf_counter() - t0
    t0 = time.perf_counter()
    y64, h64 = oracle.gru_predict_f64(oracle_weights(W_G), xs, threads=threads)
    dt64 = time.perf_counter() - t0
    per = np.abs(y - yo).max(axis=1)
    mg = _margin(y, yo, y64)
    for eng, ye in y_eng.items():
        pe = np.abs(ye - yo).max(axis=1)
        me = _margin(ye, yo, y64)
        dh, de = np.abs(y - y64).max(axis=1), np.abs(ye - y64).max(axis=1)
        _record_full(f"configs[1] GRU-HS[64] 4096 x 65536, engine {eng}", streams=B, worst=float(pe.max()), median=float(np.median(pe)),
                     p99=float(np.quantile(pe, 0.99)), margin_y=me, exact_engine_hip_vs_f64=mg["hip_vs_f64"],
                     streams_closer_to_f64_than_the_exact_engine=int((de <= dh).sum()),
                     ratio_to_exact_engine_per_stream={"worst": float((de / np.maximum(dh, 1e-12)).max()), "median": float(np.median(de / np.maximum(dh, 1e-12)))})
        assert pe.max() < TOL and me["hip_vs_f64"]["worst"] < TOL, (eng, pe.max())
    del y_eng
    _record_full("configs[1] GRU-HS[64] 4096 x 65536", streams=B, worst=float(per.max()), worst_stream=int(per.argmax()), median=float(np.median(per)),
                 p99=float(np.quantile(per, 0.99)), state_worst=float(np.abs(h - ho).max()), margin_y=mg,
                 state_hip_vs_f64=float(np.abs(h - h64).max()), state_oracle32_vs_f64=float(np.abs(ho - h64).max()),
                 oracle_seconds=dt, oracle_f64_seconds=dt64, oracle_threads=threads)
    assert per.max() < TOL and np.abs(h - ho).max() < TOL, (per.max(), int(per.argmax()))
    assert mg["hip_vs_f64"]["worst"] < TOL and mg["oracle32_vs_f64"]["worst"] < TOL      # each within the bar of the truth itself


@FULL
def test_full_size_cfg3_every_stream_against_the_oracle(ntm):
    """BASELINE configs[2] at full size: DiffDelGRU (fused step), all 4096 (signal, wow trajectory) pairs x 65 536, D = 1847:
    pre_d and y of every stream inside 1e-5 of the oracle, hidden state and delay buffer too; the fp64-mode margins of pre_d and
    y as in the configs[1] test."""
    import sys
    import time
    from helpers import oracle_weights
    sys.path.insert(0, ROOT)
    import bench
    B, T = 4096, 65536
    threads = max(1, min(32, len(os.sched_getaffinity(0))))      # (256 threads on the box were 2.7 x SLOWER than 32)
    dev0 = torch.device("cuda", 0)
    x = bench.synth_input(B, T, dev0, seed=1234)
    m = ntm.harness.build_model(W_D, max_delay_seconds=0.0335)
    d = bench.delay_trajectories(B, T, dev0, m.max_delay)
    y, pre = m.predict(x, d)
    y, pre = y.cpu().numpy()[:, 0], pre.cpu().numpy()[:, 0]
    h, buf = m.hidden[0].cpu().numpy(), m.diffdel.buffer[:, 0].cpu().numpy()
    m.kernel_variant = "bf16x3"          # round 6: the split engine under the delay line (GRU launch + streaming delay pass)
    yb, pb = m.predict(x, d)
    yb, pb = yb.cpu().numpy()[:, 0], pb.cpu().numpy()[:, 0]
    m.kernel_variant = "auto"
    xs, ds = x[:, 0].cpu().numpy(), d[:, 0].cpu().numpy()
    del x, d
    t0 = time.perf_counter()
    yo, preo, ho, bo = oracle.diffdel_predict(oracle_weights(W_D), xs, ds, m.max_delay, threads=threads)
    dt = time.perf_counter() - t0
    per_y, per_p = np.abs(y - yo).max(axis=1), np.abs(pre - preo).max(axis=1)
    t0 = time.perf_counter()
    y64, p64, _, _ = oracle.diffdel_predict_f64(oracle_weights(W_D), xs, ds, m.max_delay, threads=threads)
    dt64 = time.perf_counter() - t0
    mp = _margin(pre, preo, p64)
    mpb, myb = _margin(pb, preo, p64), _margin(yb, yo, y64)
    _record_full("configs[2] DiffDelGRU-HS[64] 4096 x 65536, D = 1847, engine bf16x3 (GRU launch + delay pass)", streams=B,
                 worst_y=float(np.abs(yb - yo).max()), worst_pre_d=float(np.abs(pb - preo).max()), margin_pre_d=mpb, margin_y=myb,
                 exact_engine_hip_vs_f64=mp["hip_vs_f64"])
    assert np.abs(yb - yo).max() < TOL and np.abs(pb - preo).max() < TOL and mpb["hip_vs_f64"]["worst"] < TOL
    del p64, preo, pb, yb
    my = _margin(y, yo, y64)
    _record_full("configs[2] DiffDelGRU-HS[64] 4096 x 65536, D = 1847 (fused step)", streams=B, worst_y=float(per_y.max()), worst_pre_d=float(per_p.max()),
                 worst_stream=int(per_p.argmax()), median_pre_d=float(np.median(per_p)), p99_pre_d=float(np.quantile(per_p, 0.99)),
                 state_worst=float(np.abs(h - ho).max()), buffer_worst=float(np.abs(buf - bo).max()), margin_pre_d=mp, margin_y=my,
                 oracle_seconds=dt, oracle_f64_seconds=dt64, oracle_threads=threads)
    assert per_y.max() < TOL and per_p.max() < TOL and np.abs(h - ho).max() < TOL and np.abs(buf - bo).max() < TOL
    assert mp["hip_vs_f64"]["worst"] < TOL and my["hip_vs_f64"]["worst"] < TOL


# ----------------------------------------------------------------------------- DiffDelGRU: both time-domain losses out of the fused step
@pytest.mark.parametrize("B,T,skip,MD", [(1040, 300, 64, 299), (1040, 4136, 1024, 1846), (4200, 700, 256, 299), (1040, 129, 128, 49),
                                         (700, 300, 64, 299), (1040, 1000, 4, 1846), (1040, 300, 2, 299)])
def test_diffdel_forward_losses_in_one_launch(ntm, B, T, skip, MD):
    """DiffDelRNN.predict_losses (ntm_diffdel_gru_forward_losses): y and pre_d bit-identical to predict(), the ESR sums
    bit-identical to predict_esr's, the DCPreESR sums of the DELAYED output against the streaming kernel on the same output
    (2e-6 rel) and the oracle (2e-5 rel); trajectories with taps in the carried history and wow; B = 700 and skip = 2 take the
    forward + streaming passes."""
    rng = np.random.default_rng(B + T + skip + MD)
    x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
    t = (0.6 * np.tanh(1.7 * np.roll(x, 7, axis=1)) + 0.04).astype(np.float32)
    n = np.arange(T)
    d = (0.5 * MD + 0.45 * MD * np.sin(n / 97.0 + rng.uniform(0, 6, (B, 1)))).astype(np.float32)
    xd, td, dd = dev(x).unsqueeze(1), dev(t).unsqueeze(1), dev(d).unsqueeze(1)
    m = ntm.DiffDelRNN(1, 64, 1, skip=False, max_delay=MD)
    m.load_state_dict(ntm.weights.load_state_dict(W_D))
    m = m.to("cuda").eval()
    y, pre, s, dc = m.predict_losses(xd, dd, td, skip=skip)
    h, buf = m.hidden.clone(), m.diffdel.buffer.clone()
    y0, p0 = m.predict(xd, dd)
    assert torch.equal(y, y0) and torch.equal(pre, p0) and torch.equal(m.hidden, h) and torch.equal(m.diffdel.buffer, buf)
    y1, p1, s1 = m.predict_esr(xd, dd, td, skip=skip)
    assert torch.equal(y1, y0) and torch.equal(s1, s)
    want = ntm.esr_dcpre_sums(y0, td, skip).cpu().numpy()
    got = dc.cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(got - want) / np.maximum(np.abs(want), 1e-30)).max() < 2e-6
    rows = [0, 15, 16, B // 2, B - 1]
    assert np.allclose(got[rows], oracle.esr_dcpre_sums(y0[rows, 0].cpu().numpy(), t[rows], skip), rtol=2e-5, atol=1e-12)


def test_cli_diffdel_evaluation_is_one_launch_for_both_time_domain_losses(tmp_path, monkeypatch):
    """The loss script's DiffDelGRU command (scripts/test-model-loss.sh:57-63 with MODEL = DiffDelGRU: --ADD_DELAY) now issues
    predict + ESR + DCPreESR as ONE call; same losses as --KERNEL mfma2, which keeps the separate passes."""
    from test_cli import _wow_dataset, cli_module
    cli = cli_module("ntm_cli_r5c")
    _wow_dataset(tmp_path, "Wow")
    monkeypatch.chdir(tmp_path)
    argv = ["--MODEL", "DiffDelGRU", "--WEIGHTS", W_D, "--DATASET_DIR", str(tmp_path / "Wow"), "--SUBSET", "Test", "--NO_SHUFFLE",
            "--SEGMENT_LENGTH", "12000", "--ADD_DELAY", "--COMPUTE_LOSS", "--NO_EXAMPLE", "--NO_CACHE", "--INIT_LEN", "2048"]
    pa, pb = {}, {}
    a = cli.main(argv, profile=pa)
    b = cli.main(argv + ["--KERNEL", "mfma2"], profile=pb)
    assert "predict+ESR+DCPreESR_ms" in pa and "ESR_ms" not in pa and "predict_ms" in pb and "ESR_ms" in pb and "DCPreESR_ms" in pb
    # (another GRU kernel underneath: the outputs differ in the last bits, the losses by far less than 1e-4)
    assert abs(a["ESR"] / b["ESR"] - 1) < 1e-4 and abs(a["DCPreESR"] / b["DCPreESR"] - 1) < 1e-4 and abs(a["MultiSTFT"] / b["MultiSTFT"] - 1) < 1e-4


def test_forward_losses_random_shapes_both_models(ntm):
    """Seeded sweep over ragged shapes for the losses-in-the-launch kernels (GRU flush and fused DiffDelGRU delay stage):
    T from 1 sample to a dozen tiles, skip anywhere a multiple of 4 up to T (incl. skip = T: empty sums), every result
    against the streaming kernels on the same output (ESR bit for bit via predict_esr, DCPreESR 3e-6 rel)."""
    rng = np.random.default_rng(505)
    mg = ntm.harness.build_model(W_G)
    md = ntm.DiffDelRNN(1, 64, 1, skip=False, max_delay=120)
    md.load_state_dict(ntm.weights.load_state_dict(W_D))
    md = md.to("cuda").eval()
    B = 1040
    for it in range(24):
        T = int(rng.choice([1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 300, 511, 640, 777]))
        skip = 4 * int(rng.integers(0, T // 4 + 1))
        x = rng.uniform(-0.5, 0.5, (B, T)).astype(np.float32)
        t = (0.5 * np.tanh(2 * x) + 0.03).astype(np.float32)
        xd, td = dev(x).unsqueeze(1), dev(t).unsqueeze(1)
        y, s, dc = mg.predict_losses(xd, td, skip=skip)
        y1, s1 = mg.predict_esr(xd, td, skip=skip)
        want = ntm.esr_dcpre_sums(y1, td, skip)
        assert torch.equal(y, y1) and torch.equal(s, s1), (T, skip)
        tol = 3e-6 * want.abs() + 1e-12
        assert bool(((dc - want).abs() <= tol).all()), ("gru", T, skip, float(((dc - want).abs() / want.abs().clamp_min(1e-30)).max()))
        d = (60.0 + 55.0 * np.sin(np.arange(T) / 23.0 + rng.uniform(0, 6, (B, 1)))).astype(np.float32)
        dd = dev(d).unsqueeze(1)
        yy, pp, ss, dcc = md.predict_losses(xd, dd, td, skip=skip)
        y2, p2, s2 = md.predict_esr(xd, dd, td, skip=skip)
        want2 = ntm.esr_dcpre_sums(y2, td, skip)
        assert torch.equal(yy, y2) and torch.equal(pp, p2) and torch.equal(ss, s2), (T, skip)
        tol2 = 3e-6 * want2.abs() + 1e-12
        assert bool(((dcc - want2).abs() <= tol2).all()), ("diffdel", T, skip, float(((dcc - want2).abs() / want2.abs().clamp_min(1e-30)).max()))
