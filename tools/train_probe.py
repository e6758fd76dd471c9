#!/usr/bin/env python3
"""Time of one TBPTT window of RNN.train_epoch (code/model.py:126-153: forward + loss + backward + Adam step) for GRU-HS[64] at
L = 1024 samples, B = 32 (code/train.py's BATCH_SIZE) and B = 4096 (a throughput point): this engine (csrc/gru_train.hip) and
torch.nn.GRU + Linear (MIOpen) on the same GPU, the latter in a fresh child process.  With --rocprof the engine's part is re-run
in a child under `rocprofv3 --kernel-trace --stats` and the per-kernel times are listed.
With --model diffdel: one TBPTT window of DiffDelRNN.train_epoch (code/model.py:464-497) for DiffDelGRU-HS[64] at L = 2048, D = 11 001
(forward: GRU + delay line, loss, backward: delay adjoint + BPTT + reduce, Adam), and the backward of a 16 384-sample warm-up
(TBPTT_INIT at that D) reached through the first window; its GRU workspace is B * 16 384 * 1280 B (0.67 GB at B = 32).
With --replicas R[,R...]: one TBPTT window of ntm_amd.Replicas (R models at B = 32 each, one launch per kernel for all of them)
beside R sequential windows of the single-model path in the same process -- whole window, window without the optimizer steps, and
the optimizer steps alone, with one optimizer per replica and with one optimizer over all parameters; median and range over
--reps repetitions of --iters windows.  GRU: L = 1024; --model diffdel: L = 2048, D = 11 001.
With --validate --replicas R[,R...]: one validation batch of the reference's shape (code/train.py:148: 6 segments of 441 000
samples) through Replicas.validate (one launch of the low-latency kernel for all R models) beside R sequential single-model
validate() calls on the same data, host time from call to return (validate ends with the losses on the host); the forms alternate
within a repetition, median and range over --reps repetitions.  --model diffdel: D = 11 001, warm-up 16 384.
With --loss esr|dcpre|mrstft (default esr) the single-model windows (plain and --model diffdel) use that loss; mrstft is
MRSTFTLoss() at its default resolutions on the 2048-sample windows of --model diffdel and without the 2048-point resolution on
the GRU's 1024-sample windows (reflect padding needs T > n_fft/2).  With mrstft the probe also lists, per resolution, the time of
ntm_stft_sums and of its adjoint ntm_stft_grad (frame kernel + gather) on a window's shape, and --rocprof shows both adjoint
kernels in the per-kernel split.
usage: python tools/train_probe.py [--model gru|diffdel] [--loss esr|dcpre|mrstft] [--iters N] [--rocprof]
                                   [--replicas 1,2,4,8 [--reps N] [--validate]]"""
import argparse
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
L = 1024


def _time(fn, iters):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def _loss_fcn(name, T):
    import ntm_amd
    if name == "mrstft":
        keep = [i for i, n in enumerate(ntm_amd.model.MRSTFT_FFT_SIZES) if T > n // 2]
        return ntm_amd.MRSTFTLoss(*([v[i] for i in keep] for v in (ntm_amd.model.MRSTFT_FFT_SIZES, ntm_amd.model.MRSTFT_HOP_SIZES,
                                                                   ntm_amd.model.MRSTFT_WIN_LENGTHS)))
    return ntm_amd.ESRLoss() if name == "esr" else ntm_amd.DCPreESR(dc_pre=True)


def stft_split(B, T, iters):
    """-> {n_fft: [ms of ntm_stft_sums, ms of ntm_stft_grad]} for the resolutions of MRSTFTLoss that fit T, by events."""
    import torch
    import ntm_amd
    lib, p = ntm_amd._lib.lib(), ntm_amd._lib.ptr
    y, t = torch.rand(B, 1, T, device="cuda") - 0.5, torch.rand(B, 1, T, device="cuda") - 0.5
    coef = torch.rand(B, 3, device="cuda")
    dy = torch.empty(B, T, device="cuda")
    out = {}
    for n_fft, hop, win in _loss_fcn("mrstft", T).resolutions:
        ws = torch.empty(lib.ntm_stft_grad_workspace_floats(B, T, 0, n_fft, hop), device="cuda")

        def grad():
            ntm_amd._lib.check(lib.ntm_stft_grad(p(y), p(t), B, T, 0, n_fft, hop, win, ntm_amd.model.STFT_EPS, p(coef), p(ws), p(dy), 0,
                                                 ntm_amd._lib.current_stream()), "ntm_stft_grad")
        out[str(n_fft)] = [_time(lambda: ntm_amd.stft_sums(y, t, 0, n_fft, hop, win), iters), _time(grad, iters)]
    return out


def engine(B, iters, loss="esr"):
    import torch
    import ntm_amd
    torch.manual_seed(0)
    m = ntm_amd.RNN(1, 64, 1).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    opt = torch.optim.Adam(m.parameters(), 1e-3)
    loss_fcn = _loss_fcn(loss, L)
    x = torch.rand(B, 1, L, device="cuda") - 0.5
    t = 0.5 * x
    m.hidden = torch.zeros(1, B, 64, device="cuda")

    def window():
        y = m(x)
        loss = loss_fcn(y, t)
        loss.backward()
        opt.step()
        m.detach_hidden()
        m.zero_grad()
    return _time(window, iters)


DD_L, DD_D, DD_INIT = 2048, 11001, 16384


def engine_diffdel(B, iters, loss="esr"):
    """-> (ms per window, ms per warm-up + first window, ms of the delay adjoint alone per window)."""
    import torch
    import ntm_amd
    torch.manual_seed(0)
    m = ntm_amd.DiffDelRNN(1, 64, 1, max_delay=DD_D - 1).cuda()
    for p in m.parameters():
        p.requires_grad_(True)
    opt = torch.optim.Adam(m.parameters(), 1e-3)
    loss_fcn = _loss_fcn(loss, DD_L)
    n = torch.arange(DD_INIT + DD_L, device="cuda", dtype=torch.float32)
    d = (5500.0 + 4000.0 * torch.sin(n / 7000.0) + 20.0 * torch.sin(n / 300.0)).expand(B, 1, -1).contiguous()
    x = torch.rand(B, 1, DD_INIT + DD_L, device="cuda") - 0.5
    t = 0.5 * x
    m.initialize_hidden(B, m.max_delay)
    m(x[:, :, :DD_INIT], d[:, :, :DD_INIT], warmup=True)
    m.detach_hidden()
    xs, ds, ts = x[:, :, DD_INIT:], d[:, :, DD_INIT:], t[:, :, DD_INIT:]

    def window():
        y, _ = m(xs, ds)
        loss = loss_fcn(y, ts)
        loss.backward()
        opt.step()
        m.detach_hidden()
        m.zero_grad()

    def first_window():
        m.initialize_hidden(B, m.max_delay)
        m(x[:, :, :DD_INIT], d[:, :, :DD_INIT], warmup=True)
        window()

    L_ = ntm_amd._lib.lib()
    gy = torch.randn(B, DD_L, device="cuda")
    dd = ds.reshape(B, DD_L).contiguous()
    gpre = torch.empty(B, DD_L, device="cuda")
    gbuf = torch.empty(B, DD_D, device="cuda")
    p = ntm_amd._lib.ptr

    def adjoint():
        ntm_amd._lib.check(L_.ntm_delay_backward(p(gy), p(dd), None, p(gpre), p(gbuf), B, DD_L, DD_D, 0, 0,
                                                 ntm_amd._lib.current_stream()), "ntm_delay_backward")
    return _time(window, iters), _time(first_window, max(iters // 4, 2)), _time(adjoint, iters)


def replicas(R, iters, reps, model="gru", B=32):
    """-> {name: [median, min, max] ms per window}: the group window (one optimizer per replica / one over all), R sequential
    single-model windows, both without the optimizer steps, and the optimizer steps alone."""
    import statistics
    import torch
    import ntm_amd
    torch.manual_seed(0)
    dd = model == "diffdel"
    T = DD_L if dd else L
    loss_fcn = ntm_amd.ESRLoss()

    def make():
        m = (ntm_amd.DiffDelRNN(1, 64, 1, max_delay=DD_D - 1) if dd else ntm_amd.RNN(1, 64, 1)).cuda()
        for p in m.parameters():
            p.requires_grad_(True)
        return m
    x = torch.rand(R * B, 1, T, device="cuda") - 0.5
    t = 0.5 * x
    n = torch.arange(T, device="cuda", dtype=torch.float32)
    d = (5500.0 + 4000.0 * torch.sin(n / 7000.0) + 20.0 * torch.sin(n / 300.0)).expand(R * B, 1, -1).contiguous()

    def group(opts_of):
        ms = [make() for _ in range(R)]
        g = ntm_amd.Replicas(ms)
        opts = opts_of(ms)
        g.initialize_hidden(B)
        g.hidden = torch.zeros(1, R * B, 64, device="cuda")

        def window(step=True):
            y = g(x, d, _share=False)[0] if dd else g(x, _share=False)
            losses = loss_fcn.replicas(y, t, R)
            losses.sum().backward()
            if step:
                for o in opts:
                    o.step()
            g.detach_hidden()
            g.zero_grad()
            return losses.tolist()
        window()                       # leaves gradients' shapes and the optimizer state in place
        return window, opts, ms

    def single():
        ms = [make() for _ in range(R)]
        opts = [torch.optim.Adam(m.parameters(), 1e-3) for m in ms]
        for m in ms:
            if dd:
                m.initialize_hidden(B, m.max_delay)
            m.hidden = torch.zeros(1, B, 64, device="cuda")

        def window(step=True):
            for r, (m, o) in enumerate(zip(ms, opts)):
                sl = slice(r * B, (r + 1) * B)
                y = m(x[sl], d[sl])[0] if dd else m(x[sl])
                loss = loss_fcn(y, t[sl])
                loss.backward()
                if step:
                    o.step()
                m.detach_hidden()
                m.zero_grad()
                loss.item()
        window()
        return window

    def steps_only(opts, ms):
        for m in ms:
            for p in m.parameters():
                p.grad = torch.zeros_like(p)

        def run():
            for o in opts:
                o.step()
        return run
    each = lambda ms: [torch.optim.Adam(m.parameters(), 1e-3) for m in ms]                       # noqa: E731
    one = lambda ms: [torch.optim.Adam([p for m in ms for p in m.parameters()], 1e-3)]          # noqa: E731
    w_each, o_each, m_each = group(each)
    w_one, o_one, m_one = group(one)
    w_single = single()
    runs = {"group": w_each, "group, one optimizer": w_one, f"{R} x single": w_single,
            "group, no step": lambda: w_each(False), f"{R} x single, no step": lambda: w_single(False),
            "steps alone": steps_only(o_each, m_each), "step alone, one optimizer": steps_only(o_one, m_one)}
    times = {name: [] for name in runs}
    for _ in range(reps):               # the forms alternate within a repetition, so that drift of the machine hits all alike
        for name, fn in runs.items():
            times[name].append(_time(fn, iters))
    return {name: [statistics.median(v), min(v), max(v)] for name, v in times.items()}


VAL_B, VAL_T = 6, 441000


class _ValLoader(list):
    """What validate() needs of a DataLoader: len(), (x, t, meta) batches, .dataset.fs / .dataset.delay_analyzer.max_delay."""

    def __init__(self, batches, fs, max_delay_s):
        super().__init__(batches)
        self.dataset = type("DS", (), {"fs": fs, "delay_analyzer": type("DA", (), {"max_delay": max_delay_s})})


def validate_probe(R, reps, model="gru", B=VAL_B, T=VAL_T):
    """-> {name: [median, min, max] ms per validation batch}: Replicas.validate of R models against R sequential validate()
    calls of the same models on the same batch (and that the two gave the same losses)."""
    import statistics
    import time
    import torch
    import ntm_amd
    torch.manual_seed(0)
    dd = model == "diffdel"
    fs = 44100
    ms = [(ntm_amd.DiffDelRNN(1, 64, 1, max_delay=DD_D - 1) if dd else ntm_amd.RNN(1, 64, 1)).cuda() for _ in range(R)]
    x = torch.rand(B, 1, T, device="cuda") - 0.5
    n = torch.arange(T, dtype=torch.float32)
    meta = {"delay_trajectory": ((5500.0 + 4000.0 * torch.sin(n / 7000.0) + 20.0 * torch.sin(n / 300.0)) / fs).expand(B, -1).contiguous().cuda()}
    loader = _ValLoader([(x, 0.5 * x, meta)], fs, (DD_D - 1) / fs)
    loss_fcn = ntm_amd.ESRLoss()
    g = ntm_amd.Replicas(ms)
    out = {}

    def group():
        out["group"] = [v for v, _ in g.validate(loader, loss_fcn, store_examples=False)]

    def single():
        out["single"] = [m.validate(loader, loss_fcn, store_examples=False)[0] for m in ms]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    runs = {"group": group, f"{R} x single": single}
    for fn in runs.values():
        fn()                            # warm-up: allocations, the first launch of every kernel
    times = {name: [] for name in runs}
    for _ in range(reps):               # the forms alternate within a repetition, so that drift of the machine hits all alike
        for name, fn in runs.items():
            times[name].append(wall(fn))
    res = {name: [statistics.median(v), min(v), max(v)] for name, v in times.items()}
    res["same losses"] = out["group"] == out["single"]
    return res


def miopen(B, iters, native=False):
    """torch.nn.GRU + Linear training; `native`: with torch's own GRU cell kernels instead of MIOpen (cudnn backend off)."""
    import torch
    torch.backends.cudnn.enabled = not native
    torch.manual_seed(0)
    gru = torch.nn.GRU(1, 64, batch_first=True).cuda()
    lin = torch.nn.Linear(64, 1).cuda()
    opt = torch.optim.Adam(list(gru.parameters()) + list(lin.parameters()), 1e-3)
    x = torch.rand(B, L, 1, device="cuda") - 0.5
    t = 0.5 * x
    state = {"h": torch.zeros(1, B, 64, device="cuda")}

    def window():
        out, h = gru(x, state["h"])
        y = lin(out)
        loss = ((t - y) ** 2).mean() / ((t ** 2).mean() + 1e-5)
        loss.backward()
        opt.step()
        state["h"] = h.detach()
        opt.zero_grad()
    return _time(window, iters)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--child", choices=["engine", "miopen", "native", "diffdel", "replicas", "validate", "stft"])
    ap.add_argument("--loss", choices=["esr", "dcpre", "mrstft"], default="esr", help="loss of the single-model windows")
    ap.add_argument("--replicas", default=None, help="comma-separated replica counts, e.g. 1,2,4,8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="32,4096")
    ap.add_argument("--model", choices=["gru", "diffdel"], default="gru")
    ap.add_argument("--validate", action="store_true", help="with --replicas: one grouped validation batch against R single ones")
    a = ap.parse_args()
    sizes = [int(b) for b in a.sizes.split(",")]
    if a.child == "diffdel":
        print(json.dumps({str(B): engine_diffdel(B, a.iters, a.loss) for B in sizes}))
        return
    if a.child == "stft":
        print(json.dumps({str(B): stft_split(B, DD_L if a.model == "diffdel" else L, a.iters) for B in sizes}))
        return
    if a.child == "validate":
        print(json.dumps({str(R): validate_probe(R, a.reps, a.model) for R in map(int, a.replicas.split(","))}))
        return
    if a.child == "replicas":
        print(json.dumps({str(R): replicas(R, a.iters, a.reps, a.model) for R in map(int, a.replicas.split(","))}))
        return
    if a.child:
        out = {}
        for B in sizes:
            if a.child == "engine":
                out[str(B)] = engine(B, a.iters, a.loss)
                continue
            # a torch-side RuntimeError (e.g. a MIOpen status) is reported as data: the child still exits normally, so that the
            # parent can tell it from a crash
            try:
                out[str(B)] = miopen(B, a.iters, native=a.child == "native")
            except RuntimeError as e:
                out[str(B)] = f"error: {str(e).splitlines()[0][:200]}"
        print(json.dumps(out))
        return

    def child(cmd, what):
        """Run one GPU child; anything but a clean exit (a Python error, a signal, an abort, a time limit) ends the probe before
        another GPU process is started."""
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"{what}: time limit; nothing more is started")
        if r.returncode != 0:
            raise SystemExit(f"{what} exited with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
        return r

    if a.replicas and a.validate:
        r = child([sys.executable, __file__, "--child", "validate", "--replicas", a.replicas, "--reps", str(a.reps), "--model", a.model],
                  "validate child")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        what = f"DiffDelGRU-HS[64], D = {DD_D}" if a.model == "diffdel" else "GRU-HS[64]"
        print(f"{what}, one validation batch of {VAL_B} x {VAL_T} per replica (ESRLoss); ms from call to return, median [min .. max] "
              f"of {a.reps} repetitions:")
        for R, rows in res.items():
            same = rows.pop("same losses")
            print(f"R = {R}   (grouped losses == single losses: {same})")
            for name, (med, lo, hi) in rows.items():
                print(f"  {name:<28} {med:9.2f}  [{lo:.2f} .. {hi:.2f}]")
        if a.rocprof:
            for R in a.replicas.split(","):
                _rocprof(child, a, [R], "validate", ["--replicas", R, "--reps", "1", "--model", a.model])
        return

    if a.replicas:
        r = child([sys.executable, __file__, "--child", "replicas", "--replicas", a.replicas, "--iters", str(a.iters), "--reps",
                   str(a.reps), "--model", a.model], "replicas child")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        what = f"DiffDelGRU-HS[64], L = {DD_L}, D = {DD_D}" if a.model == "diffdel" else f"GRU-HS[64], L = {L}"
        print(f"{what}, B = 32 per replica; ms per window, median [min .. max] of {a.reps} x {a.iters} windows:")
        for R, rows in res.items():
            print(f"R = {R}")
            for name, (med, lo, hi) in rows.items():
                print(f"  {name:<28} {med:8.3f}  [{lo:.3f} .. {hi:.3f}]")
        if a.rocprof:
            for R in a.replicas.split(","):
                _rocprof(child, a, [R], "replicas", ["--replicas", R, "--reps", "1", "--model", a.model])
        return

    def stft_rows():
        if a.loss != "mrstft":
            return
        r = child([sys.executable, __file__, "--child", "stft", "--iters", str(a.iters), "--sizes", a.sizes, "--model", a.model], "stft child")
        print(f"\nper resolution on a window's shape, ms: {'B':>6} {'n_fft':>6} {'ntm_stft_sums':>14} {'ntm_stft_grad':>14}")
        for B, rows in json.loads(r.stdout.strip().splitlines()[-1]).items():
            for n_fft, (fwd, adj) in rows.items():
                print(f"{'':<39} {B:>6} {n_fft:>6} {fwd:14.4f} {adj:14.4f}")

    extra = ["--loss", a.loss]
    if a.model == "diffdel":
        r = child([sys.executable, __file__, "--child", "diffdel", "--iters", str(a.iters), "--sizes", a.sizes] + extra, "diffdel child")
        res = json.loads(r.stdout.strip().splitlines()[-1])
        print(f"DiffDelGRU-HS[64], ms (L = {DD_L}, D = {DD_D}; window = forward + {a.loss} loss + backward + Adam):")
        print(f"{'B':>6} {'window':>9} {'warm-up + window 1':>19} {'delay adjoint':>14} {'adjoint share':>14}")
        for B in map(str, sizes):
            w, f, adj = res[B]
            print(f"{B:>6} {w:9.3f} {f:19.3f} {adj:14.4f} {adj / w * 100:13.2f}%")
        stft_rows()
        if a.rocprof:
            _rocprof(child, a, sizes, "diffdel", extra)
        return

    rows = {}
    for kind in ("engine", "miopen", "native"):
        if kind != "engine" and a.loss != "esr":
            rows[kind] = {str(B): None for B in sizes}           # the torch baselines are written for the ESR loss only
            continue
        r = child([sys.executable, __file__, "--child", kind, "--iters", str(a.iters), "--sizes", a.sizes] + extra, f"{kind} child")
        rows[kind] = json.loads(r.stdout.strip().splitlines()[-1])
    fmt = lambda v: f"{v:.3f}" if isinstance(v, float) else "n/a"      # noqa: E731
    print(f"ms per TBPTT window (L = 1024; forward + {a.loss} loss + backward + Adam):")
    print(f"{'B':>6} {'this engine':>12} {'MIOpen':>10} {'torch native':>13}")
    for B in map(str, sizes):
        print(f"{B:>6} {fmt(rows['engine'][B]):>12} {fmt(rows['miopen'][B]):>10} {fmt(rows['native'][B]):>13}")
    for kind in ("miopen", "native"):
        for B in map(str, sizes):
            if isinstance(rows[kind][B], str):
                print(f"  {kind} B={B}: {rows[kind][B]}")
    stft_rows()
    if a.rocprof:
        _rocprof(child, a, sizes, "engine", extra)


def _rocprof(child, a, sizes, kind, extra=()):
    """The per-kernel split of the `kind` child under rocprofv3 --kernel-trace --stats, one child per batch size."""
    import csv
    for B in sizes:
        with tempfile.TemporaryDirectory() as d:
            child(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "probe", "--output-format", "csv", "--", sys.executable,
                   __file__, "--child", kind, "--iters", str(a.iters), "--sizes", str(B), *extra], f"rocprofv3 {kind} child B={B}")
            stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not stats:
                raise SystemExit("rocprofv3 wrote no kernel stats")
            krows = list(csv.DictReader(open(stats[0])))
        total = sum(float(x["TotalDurationNs"]) for x in krows)
        print(f"\nper-kernel time of the {kind} child at {'R' if kind in ('replicas', 'validate') else 'B'} = {B} (all of its windows):")
        for x in sorted(krows, key=lambda x: -float(x["TotalDurationNs"]))[:12]:
            print(f"{float(x['TotalDurationNs']) / total * 100:6.1f}%  {int(x['Calls']):6d} calls  "
                  f"{float(x['AverageNs']) / 1e3:10.1f} us avg  {x['Name'][:90]}")


if __name__ == "__main__":
    main()
