"""GPU: the device spectrogram (ntm_spectrogram), its adjoint (ntm_spectrogram_grad), training.SpectrogramFn and
TimeFreqConverter (csrc/stft_kernels.hip).

The reference everywhere is torch.stft on the CPU in float64 as helpers._torch_power forms it, with torch autograd for the
gradients; ref32 is the same graph in float32 on the CPU.  The bar of every comparison, elementwise:

    bar = 4 * max(|ref32 - ref64|, E32(n_fft) * max|ref64|)

E32(n_fft) is the worst max|ref32 - ref64| / max|ref64| over that n_fft's case table (forward and adjoint each their own),
computed here from the two torch references.  The factor 4 is the project's margin over torch's own float32 (DESIGN.md 11,
11.4); the quantity is smooth, so there is no conditioning allowance.  The cases are helpers.structural_cases(n_fft) with
`skip` dropped (T = L).  The references are computed once per n_fft and shared.

Measured on an MI355X, worst |got - ref64| / bar per n_fft: see DESIGN.md 11.5."""
import functools

import numpy as np
import pytest
import torch

from helpers import _torch_power, noise_pair, structural_cases

N_FFTS = [64, 128, 256, 512, 1024, 2048]


@pytest.fixture(scope="module")
def ntm():
    import ntm_amd
    assert torch.cuda.is_available(), "these tests need the MI355X"
    ntm_amd._lib.lib()
    return ntm_amd


# ---- references -----------------------------------------------------------------------------------------------------
def cases(n_fft):
    """[(T, hop, win, B)] of helpers.structural_cases without the skip."""
    return [(L, hop, win, B) for L, hop, win, _, B in structural_cases(n_fft)]


def signal(n_fft, j, B, T):
    return noise_pair(1000 * n_fft + j, B, T)[0]


def upstream(n_fft, j, B, T, hop):
    """Standard normal gP (B, bins, frames) float32."""
    return np.random.default_rng(77 * n_fft + j).standard_normal((B, n_fft // 2 + 1, 1 + T // hop)).astype(np.float32)


def ref_grad(y, gP, n_fft, hop, win, dtype):
    """d/dy sum(gP * |stft(y)|^2) by torch autograd in `dtype` -> (B, T) float64 numpy."""
    yy = torch.from_numpy(y).to(dtype).requires_grad_(True)
    X = torch.stft(yy, n_fft, hop, win, torch.hann_window(win, dtype=dtype), return_complex=True)
    ((X.real ** 2 + X.imag ** 2) * torch.from_numpy(gP).to(dtype)).sum().backward()
    return yy.grad.double().numpy()


def _e32(pairs):
    return max(float(np.abs(r32 - r64).max()) / float(np.abs(r64).max()) for r64, r32 in pairs)


@functools.lru_cache(maxsize=None)
def forward_table(n_fft):
    """([(case, y, P64, P32)], E32) -- computed once, never written to."""
    rows = []
    for j, (T, hop, win, B) in enumerate(cases(n_fft)):
        y = signal(n_fft, j, B, T)
        rows.append(((T, hop, win, B), y, _torch_power(y, n_fft, hop, win, torch.float64).numpy(),
                     _torch_power(y, n_fft, hop, win, torch.float32).double().numpy()))
    return rows, _e32([(r[2], r[3]) for r in rows])


@functools.lru_cache(maxsize=None)
def adjoint_table(n_fft):
    """([(case, y, gP, g64, g32)], E32)."""
    rows = []
    for j, (T, hop, win, B) in enumerate(cases(n_fft)):
        y, gP = signal(n_fft, j, B, T), upstream(n_fft, j, B, T, hop)
        rows.append(((T, hop, win, B), y, gP, ref_grad(y, gP, n_fft, hop, win, torch.float64),
                     ref_grad(y, gP, n_fft, hop, win, torch.float32)))
    return rows, _e32([(r[3], r[4]) for r in rows])


def check(got, r64, r32, e32, what):
    """Elementwise |got - ref64| <= 4 max(|ref32 - ref64|, E32 max|ref64|) -> the worst error / bar."""
    got = np.asarray(got, np.float64)
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    bar = 4.0 * np.maximum(np.abs(r32 - r64), e32 * float(np.abs(r64).max()))
    ratio = np.abs(got - r64) / bar
    worst = float(ratio.max())
    print(f"{what}: worst err / bar {worst:.3f}   max err {float(np.abs(got - r64).max()):.3e}   max|ref64| {float(np.abs(r64).max()):.3e}")
    assert np.isfinite(got).all() and worst <= 1.0, (what, worst)
    return worst


# ---- the raw entry points -------------------------------------------------------------------------------------------
def raw_forward(ntm, y, n_fft, hop, win):
    """ntm_spectrogram on a numpy (B, T) float32 -> device tensor (B, bins, frames); every cell starts as NaN."""
    L = ntm._lib.lib()
    yd = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    B, T = y.shape
    P = torch.full((B, n_fft // 2 + 1, 1 + T // hop), float("nan"), device="cuda")
    rc = L.ntm_spectrogram(ntm._lib.ptr(yd), B, T, n_fft, hop, win, ntm._lib.ptr(P), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error().decode()
    torch.cuda.synchronize()
    return P


def raw_adjoint(ntm, y, gP, n_fft, hop, win, dy0=None):
    """ntm_spectrogram_grad on numpy inputs -> device tensor (B, T); dy0 given: accumulate onto it."""
    L = ntm._lib.lib()
    p = ntm._lib.ptr
    yd, gd = torch.from_numpy(np.ascontiguousarray(y)).cuda(), torch.from_numpy(np.ascontiguousarray(gP)).cuda()
    B, T = y.shape
    n = L.ntm_stft_grad_workspace_floats(B, T, 0, n_fft, hop)
    assert n == B * (1 + T // hop) * n_fft and gP.shape == (B, n_fft // 2 + 1, 1 + T // hop)
    ws = torch.full((n,), float("nan"), device="cuda")
    dy = torch.full((B, T), float("nan"), device="cuda") if dy0 is None else torch.from_numpy(dy0).cuda()
    rc = L.ntm_spectrogram_grad(p(yd), p(gd), B, T, n_fft, hop, win, p(ws), p(dy), int(dy0 is not None), ntm._lib.current_stream())
    assert rc == 0, L.ntm_last_error().decode()
    torch.cuda.synchronize()
    return dy


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft", N_FFTS)
def test_forward_against_float64_stft(ntm, n_fft):
    rows, e32 = forward_table(n_fft)
    worst = 0.0
    for (T, hop, win, B), y, p64, p32 in rows:
        got = raw_forward(ntm, y, n_fft, hop, win)
        assert got.shape == (B, n_fft // 2 + 1, 1 + T // hop)
        worst = max(worst, check(got.cpu().numpy(), p64, p32, e32, f"forward n_fft {n_fft} T {T} hop {hop} win {win} B {B}"))
    print(f"forward n_fft {n_fft}: E32 {e32:.3e}, worst err / bar over {len(rows)} cases = {worst:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft", N_FFTS)
def test_adjoint_against_float64_autograd(ntm, n_fft):
    rows, e32 = adjoint_table(n_fft)
    worst = 0.0
    for (T, hop, win, B), y, gP, g64, g32 in rows:
        got = raw_adjoint(ntm, y, gP, n_fft, hop, win)
        worst = max(worst, check(got.cpu().numpy(), g64, g32, e32, f"adjoint n_fft {n_fft} T {T} hop {hop} win {win} B {B}"))
    print(f"adjoint n_fft {n_fft}: E32 {e32:.3e}, worst err / bar over {len(rows)} cases = {worst:.3f}")


# one case each: an odd and an even frame count, a hop that does not divide T, a window shorter than the frame
ONE_HOT_CASES = {64: (150, 16, 60, 1), 1024: (2100, 256, 1023, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft", [64, 1024])
def test_adjoint_of_a_one_hot_upstream_and_accumulate(ntm, n_fft):
    """A wrong once / twice factor on the DC or the Nyquist bin shows here and nowhere else."""
    T, hop, win, B = ONE_HOT_CASES[n_fft]
    frames = 1 + T // hop
    _, e32 = adjoint_table(n_fft)
    y = signal(n_fft, 99, B, T)
    outs = {}
    for k, f in ((0, 0), (n_fft // 2, frames - 1), (n_fft // 4 + 3, frames // 2)):
        gP = np.zeros((B, n_fft // 2 + 1, frames), np.float32)
        gP[0, k, f] = 1.0
        g64, g32 = (ref_grad(y, gP, n_fft, hop, win, dt) for dt in (torch.float64, torch.float32))
        assert np.abs(g64).max() > 0
        got = raw_adjoint(ntm, y, gP, n_fft, hop, win)
        check(got.cpu().numpy(), g64, g32, e32, f"one-hot n_fft {n_fft} bin {k} frame {f}")
        outs[(k, f)] = (gP, got)
    gP, a = outs[(0, 0)]
    dy0 = np.random.default_rng(1).standard_normal((B, T)).astype(np.float32)
    acc = raw_adjoint(ntm, y, gP, n_fft, hop, win, dy0=dy0.copy())
    assert torch.equal(acc, torch.from_numpy(dy0).cuda() + a)                  # dy = dy + gradient, one fp32 addition per sample


# (n_fft, hop, win, T): odd and even frame counts; the last has 12 801 frames = 401 iterations of a workgroup, which the launcher
# splits into 201 chunks for the batch of 3 and into 401 for a stream alone
PROP_CASES = [(64, 16, 60, 149), (128, 33, 128, 300), (512, 128, 511, 1100), (2048, 512, 2048, 5000), (64, 1, 64, 12800)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_fft,hop,win,T", PROP_CASES)
def test_equal_calls_equal_bits_and_a_stream_does_not_depend_on_its_batch(ntm, n_fft, hop, win, T):
    B = 3
    y = signal(n_fft, 7, B, T)
    gP = upstream(n_fft, 7, B, T, hop)
    P1, P2 = raw_forward(ntm, y, n_fft, hop, win), raw_forward(ntm, y, n_fft, hop, win)
    g1, g2 = raw_adjoint(ntm, y, gP, n_fft, hop, win), raw_adjoint(ntm, y, gP, n_fft, hop, win)
    assert bool(torch.isfinite(P1).all()) and bool(torch.isfinite(g1).all())
    assert torch.equal(P1, P2) and torch.equal(g1, g2)
    assert torch.equal(raw_forward(ntm, y[1:2], n_fft, hop, win), P1[1:2])
    assert torch.equal(raw_adjoint(ntm, y[1:2], gP[1:2], n_fft, hop, win), g1[1:2])


# ---- the module -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_time_freq_converter_shapes_mel_and_gradient(ntm):
    n_fft, T = 256, 1000
    tf = ntm.TimeFreqConverter(n_fft, hop_length=100, win_length=200, n_mel_channels=40).cuda()
    y = signal(n_fft, 5, 3, T)
    x = torch.from_numpy(y).cuda().unsqueeze(1)
    P = tf(x)
    assert P.shape == (3, n_fft // 2 + 1, 1 + T // (n_fft // 4)) and not P.requires_grad and P.grad_fn is None
    assert torch.equal(P, raw_forward(ntm, y, n_fft, n_fft // 4, n_fft))            # hop n_fft / 4, window n_fft
    one = tf(x[:1])
    assert one.shape == (n_fft // 2 + 1, 1 + T // (n_fft // 4)) and torch.equal(one, P[0])
    assert tf(x[:, 0]).shape == P.shape and tf(x.reshape(3, 1, 1, T)).shape == P.shape
    Pm, mel = tf(x, mel=True)
    assert torch.equal(Pm, P) and mel.shape == (3, 40, P.shape[-1])
    # fp32 matmul: |error| <= n u sum |a| |b| with n = bins terms
    want = tf.mel_basis.double().cpu() @ P.double().cpu()
    bound = (n_fft // 2 + 1) * 2.0 ** -24 * (tf.mel_basis.double().abs().cpu() @ P.double().abs().cpu())
    assert bool(((mel.double().cpu() - want).abs() <= bound).all()) and float(mel.max()) > 0
    with torch.no_grad():
        assert not tf(x.clone().requires_grad_(True)).requires_grad
    xg = x.clone().requires_grad_(True)
    Pg = tf(xg)
    assert Pg.requires_grad and torch.equal(Pg.detach(), P)
    Pg.sum().backward()
    ones = np.ones(tuple(P.shape), np.float32)
    g64, g32 = (ref_grad(y, ones, n_fft, n_fft // 4, n_fft, dt) for dt in (torch.float64, torch.float32))
    check(xg.grad[:, 0].cpu().numpy(), g64, g32, adjoint_table(n_fft)[1], "TimeFreqConverter P.sum().backward()")
    # through the mel projection as well: torch's matmul backward feeds the node
    xm = x.clone().requires_grad_(True)
    tf(xm, mel=True)[1].sum().backward()
    gm = tf.mel_basis.sum(dim=0).cpu().numpy()[None, :, None] * ones
    g64, g32 = (ref_grad(y, gm.astype(np.float32), n_fft, n_fft // 4, n_fft, dt) for dt in (torch.float64, torch.float32))
    check(xm.grad[:, 0].cpu().numpy(), g64, g32, adjoint_table(n_fft)[1], "TimeFreqConverter mel.sum().backward()")


W_D = "DiffDelGRU-HS[64]-L[DCPreESR]-DS[ReelToReel_Dataset_MiniPulse100_CHOWTAPE_WOWFLUTTER]_BEST"
STEP_B, STEP_T0, STEP_T1, STEP_N_FFT = 2, 256, 1024, 256


def _power_t(s, n_fft):
    """helpers._torch_power's formula on a torch tensor that may require grad (hop n_fft / 4, window n_fft)."""
    X = torch.stft(s, n_fft, n_fft // 4, n_fft, torch.hann_window(n_fft, dtype=s.dtype), return_complex=True)
    return X.real ** 2 + X.imag ** 2


def _head(y, power, w, b):
    """The smooth critic-shaped head: -mean(conv1d(log10(P + 1e-5)))."""
    return -torch.nn.functional.conv1d(torch.log10(power(y) + 1e-5), w, b).mean()


@functools.lru_cache(maxsize=None)
def generator_step(ntm):
    """DiffDelRNN(1, 64, 1, max_delay=64) with the shipped DiffDelGRU-HS[64] generator weights (a generator whose output follows
    its full-scale input, as in the adversarial run), B = 2: a warm-up of 256 samples, then one window of 1024 with a delay
    trajectory inside [0, 64] samples, whose output goes through TimeFreqConverter(256) -> log10(P + 1e-5) -> a fixed random
    conv1d(129 -> 4, k = 3) -> -mean() -> backward().  Run twice -> [(y, dL/dy, parameter gradients)] and the head's weights."""
    B, T0, T1, n_fft = STEP_B, STEP_T0, STEP_T1, STEP_N_FFT
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 1, T0 + T1, generator=g) - 0.5
    n = torch.arange(T0 + T1, dtype=torch.float64)
    d = (32.0 + 30.0 * torch.sin(2 * np.pi * n / 700 + torch.rand(B, 1, generator=g, dtype=torch.float64) * 6)).float().unsqueeze(1)
    assert float(d.min()) >= 0.0 and float(d.max()) <= 64.0
    w, b = torch.randn(4, n_fft // 2 + 1, 3, generator=g) / 20.0, torch.randn(4, generator=g)
    tf = ntm.TimeFreqConverter(n_fft).cuda()
    sd = {k: torch.as_tensor(v) for k, v in ntm.weights.load_state_dict(W_D).items()}
    runs = []
    for _ in range(2):
        m = ntm.DiffDelRNN(1, 64, 1, max_delay=64).cuda()
        m.load_state_dict(sd)
        for p in m.parameters():
            p.requires_grad_(True)
        m.initialize_hidden(B, m.max_delay)
        m(x[:, :, :T0].cuda(), d[:, :, :T0].cuda(), warmup=True)
        y, _ = m(x[:, :, T0:].cuda(), d[:, :, T0:].cuda())
        y.retain_grad()
        _head(y, tf, w.cuda(), b.cuda()).backward()
        runs.append((y.detach().cpu(), y.grad.cpu(), [p.grad.clone() for p in m.parameters()]))
    return runs, w, b


@pytest.mark.gpu
def test_generator_step_gradient_at_y_against_float64(ntm):
    """(a) The gradient that reaches y, against the same head in float64 (and float32) on the CPU at the device's own y.

    The head's gP = w / ((P + 1e-5) ln 10) spans powers from 2e-5 to 5e3 in this window and multiplies the absolute error of Y at
    a cell of small power by up to 1 / (P + 1e-5): this is the comparison that needs the fp64 arithmetic inside the kernels
    (measured on an MI355X: 0.035 of the bar; the packed-fp32 transform of the sums kernels was at 8.0)."""
    runs, w, b = generator_step(ntm)
    y, gy, _ = runs[0]
    assert y.shape == (STEP_B, 1, STEP_T1) and float(y.abs().max()) > 0.1
    refs = []
    for dt in (torch.float64, torch.float32):
        yy = y[:, 0].to(dt).clone().requires_grad_(True)
        _head(yy, lambda s: _power_t(s, STEP_N_FFT), w.to(dt), b.to(dt)).backward()
        refs.append(yy.grad.double().numpy())
    err, e32 = float(np.abs(gy[:, 0].double().numpy() - refs[0]).max()), float(np.abs(refs[1] - refs[0]).max())
    print(f"critic head: max |got - ref64| {err:.3e}, max |ref32 - ref64| {e32:.3e} (ratio {err / e32:.2f}), max|ref64| {float(np.abs(refs[0]).max()):.3e}")
    check(gy[:, 0].numpy(), refs[0], refs[1], adjoint_table(STEP_N_FFT)[1], "critic head: d/dy")


@pytest.mark.gpu
def test_generator_step_parameter_gradients_are_finite_nonzero_and_reproducible(ntm):
    """(b) every parameter gradient finite and non-zero (DiffDelRNN's head is bias-free: the model has five parameter tensors,
    all of them checked), (c) a second identical run gives the same bits."""
    (_, gy1, g1), (_, gy2, g2) = generator_step(ntm)[0]
    assert len(g1) == 5
    for a in g1:
        assert bool(torch.isfinite(a).all()) and bool(a.any())
    assert torch.equal(gy1, gy2) and all(torch.equal(a, c) for a, c in zip(g1, g2))
