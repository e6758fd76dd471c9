"""The model-driving part of the reference's evaluation CLI (code/test-model.py:192-247, :296-418)
on in-memory segments: build the model from the weights-directory name, predict, cut INIT_LEN,
per-segment loss, mean over segments -- batched over streams and sharded over ranks instead of the
reference's BATCH_SIZE = 1 python loop (code/test-model.py:115,332)."""
import torch

from . import distributed, weights
from .model import RNN, DiffDelRNN, MRSTFTLoss, esr_dcpre_sums, esr_sums, ESR_EPS
from .utilities import nextpow2, parse_hidden_size, parse_loss, parse_model


def build_model(weight_name, max_delay_seconds=0.0, fs=44100, device="cuda", state_dict=None, warm_cache=True):
    """code/test-model.py:197-233: parse the directory name, construct, load best.pth.  The evaluation path never touches the
    parameters again, so the warm-start state is kept per parameter version (`warm_cache`, model.py's docstring)."""
    hidden_size = parse_hidden_size(weight_name)
    model_type = parse_model(weight_name)
    parse_loss(weight_name)                     # raises on a malformed name, as the reference would
    if model_type == "GRU":
        model = RNN(input_size=1, hidden_size=hidden_size, output_size=1, skip=False)
    elif model_type == "DiffDelGRU":
        max_delay_n = int(1.25 * max_delay_seconds * fs)          # code/test-model.py:223
        if max_delay_n == 0:
            max_delay_n = 2**8
        model = DiffDelRNN(input_size=1, hidden_size=hidden_size, output_size=1, skip=False,
                           max_delay=max_delay_n)
    else:
        raise SystemExit('Something is not right!')               # code/test-model.py:232
    model.load_state_dict(state_dict if state_dict is not None else weights.load_state_dict(weight_name))
    model = model.to(device).eval()
    model.warm_cache = bool(warm_cache)
    return model


def init_len(max_delay_seconds, fs=44100):
    """INIT_LEN = nextpow2(int(max_delay * fs))  (code/test-model.py:323-324)."""
    return nextpow2(int(max_delay_seconds * fs))


@torch.no_grad()
def compute_loss(model, input, target, d_traj=None, INIT_LEN=1024):
    """code/test-model.py:332-398 for the ESR entry of the loss dict.  input/target (B,1,T) on this
    rank (its shard of the segments); d_traj (B,1,T) in samples for DiffDelGRU.
    Returns the job-wide dict of distributed.reduce_loss_sums plus this rank's output tensor."""
    if isinstance(model, DiffDelRNN):
        output, _, s = model.predict_esr(input, d_traj, target, skip=INIT_LEN)   # cut first INIT_LEN samples (:367-369)
    else:
        output, s = model.predict_esr(input, target, skip=INIT_LEN)     # the ESR sums ride in the recurrent launch
    n = input.shape[-1] - INIT_LEN
    per_seg = (s[:, 0] / n) / (s[:, 1] / n + ESR_EPS)
    res = distributed.reduce_loss_sums(per_seg, s)
    res["ESR"] = res.pop("mean_segment_loss")
    # the DCPreESR entry of the loss dict (code/test-model.py:252): same aggregation on DC-blocked signals
    sd = esr_dcpre_sums(output, target, skip=INIT_LEN)
    res["DCPreESR"] = distributed.reduce_loss_sums((sd[:, 0] / n) / (sd[:, 1] / n + ESR_EPS))["mean_segment_loss"]
    # the MultiSTFT entry (code/test-model.py:253), when the segments are long enough for its largest frame
    if n > 1024:
        res["MultiSTFT"] = distributed.reduce_loss_sums(MRSTFTLoss().per_segment(output, target, skip=INIT_LEN))["mean_segment_loss"]
    return res, output


@torch.no_grad()
def apply_delay(delay, delay_trajectory, output, segment_length=None):
    """code/test-model.py:259-290 (`--ADD_DELAY` with `--MODEL GRU`), in working order: the reference
    calls `delay.init_buffer(N)` without the `max_d` argument its own class requires
    (code/model.py:326) and therefore raises TypeError; here the buffer is re-initialised to zeros with
    the delay line's current max_delay, then the trajectory is applied -- in one launch, or in the
    reference's 4096-sample chunks when `segment_length=2**12` (same numbers, state is carried)."""
    delay.init_buffer(output.shape[0], delay.max_delay)
    if segment_length is None:
        return delay(output, delay_trajectory)
    T = output.shape[-1]
    out = torch.empty(output.shape, device=output.device, dtype=torch.float32)
    for i in range(-(-T // segment_length)):
        sl = slice(i * segment_length, (i + 1) * segment_length)
        out[:, :, sl] = delay(output[:, :, sl], delay_trajectory[:, :, sl])
    return out


class BlockStreamer:
    """Block-by-block (real-time style) inference: B streams advance `block` samples per call with the GRU state kept
    on the device in preallocated buffers; one ctypes call per block on the low-latency kernel.  Measured on the
    MI355X (tools/attic/block_latency_probe.py): 20 us per 64-sample block of one stream (16 us of it kernel; the block
    lasts 1451 us at 44.1 kHz), 36 us for 16 streams x 128 samples, 132 us for 256 x 512 -- i.e. about 5 us of
    launch overhead.  Capturing the launch in a HIP graph and replaying it (`use_graph=True`, torch.cuda.CUDAGraph)
    was measured too and is SLOWER by 8 us per block: with a single kernel per block there is nothing for a graph to
    amortise, so it is off by default.  Same numbers as model.forward() on the concatenated blocks either way.

        s = BlockStreamer(model, B=16, block=128)          # warm-start included unless warm=False
        y = s.process(x_block)                             # (B,1,block) in -> (B,1,block) view, valid until the next call

    A DiffDelRNN streams the same way, with the delay trajectory of the block beside the audio:

        y = s.process(x_block, d_block)                    # d_block (B,1,block) in SAMPLES, what DiffDelRNN.forward takes
        y = s.process(x_block, d_block, warmup=True)       # the warm-up call of DiffDelRNN.forward: y = pre_d, the state moves on
        s.raise_if_violated()                              # the delay-range assert, one synchronisation, whenever the caller likes
        hidden, buffer = s.export_state()                  # (1,B,H), (B,1,D): what the model would carry after the same calls

    For hidden size 64 (input / output size 1, no skip connection) a block is ONE launch (csrc/diffdel_stream.hip): the
    low-latency recurrence, and the delay line on a per-stream ring in device memory whose position lives on the device too
    -- O(block) floats of delay state move per stream and call where DiffDelRNN.forward rewrites the whole buffer, and nothing
    is allocated.  y, `s.pre` (pre_d) and the exported state are the bits of model.forward() block by block with
    kernel_variant "lat" and delay_mode "two_pass" (what "auto" runs up to 1024 streams).  Every other hidden size runs
    ntm_diffdel_gru_forward per block on preallocated buffers: the GRU launch and the delay pass with its shifted buffer, the
    bits of model.forward().  tools/stream_probe.py measures both beside the RNN streamer.

    The streamer owns its state (hidden, delay line, range flag): seeded from model.hidden / model.diffdel.buffer when both are
    set for B streams (a model that has been running), else from initialize_hidden(B, model.max_delay) -- plus the model's
    warm_start(), one stream broadcast to B as in predict(), unless warm=False.  process() never touches the model's state.
    After a delay above the delay line's length (raise_if_violated() raises AssertionError, as the model does) the
    streamer's outputs and state are unspecified: build a new one.
    """

    def __init__(self, model, B, block, warm=True, use_graph=False):
        from . import _lib
        from ._lib import ptr
        self.graph = None
        if isinstance(model, DiffDelRNN):
            self._init_diffdel(model, B, block, warm, use_graph)
            return
        if not isinstance(model, RNN):
            raise TypeError("BlockStreamer drives the GRU models (RNN, DiffDelRNN)")
        self.diffdel = False
        dev = model.GRU.weight_hh_l0.device
        self.model, self.B, self.block = model, B, block
        self.x = torch.zeros(B, 1, block, device=dev, dtype=torch.float32)
        self.y = torch.empty(B, 1, block, device=dev, dtype=torch.float32)
        if warm:
            model.initialize_hidden()
            model.warm_start()
            self.h = model.hidden.expand(1, B, model.hidden_size).contiguous().clone()
        else:
            self.h = torch.zeros(1, B, model.hidden_size, device=dev, dtype=torch.float32)
        g, o = model.GRU, model.output
        lib, variant = _lib.lib(), _lib.VARIANTS[model.kernel_variant]

        def launch():
            rc = lib.ntm_gru_forward_ex(ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0),
                                        ptr(o.weight), ptr(o.bias), model.hidden_size, ptr(self.x), ptr(self.y), B, block,
                                        block, block, ptr(self.h), variant, _lib.current_stream())
            _lib.check(rc, "ntm_gru_forward")

        self._launch = launch
        if use_graph:
            h0 = self.h.clone()
            self._capture(dev, launch, lambda: self.h.copy_(h0))

    def _capture(self, dev, launch, restore):
        """Capture launch() into self.graph; restore() puts back the state a launch moves on."""
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            launch()                                        # warm the code path outside the capture
        torch.cuda.current_stream().wait_stream(side)
        restore()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            launch()
        restore()                                           # capture does not execute, but keep the state explicit

    def _init_diffdel(self, model, B, block, warm, use_graph):
        from . import _lib
        from ._lib import ptr
        if model.input_size != 1 or model.output_size != 1 or model.skip:
            raise ValueError("BlockStreamer: DiffDelRNN streams with input_size = output_size = 1 and no skip connection")
        dev = model.GRU.weight_hh_l0.device
        H = model.hidden_size
        dl = model.diffdel
        self.model, self.B, self.block, self.diffdel = model, B, block, True
        self.x = torch.zeros(B, 1, block, device=dev, dtype=torch.float32)
        self.d = torch.zeros(B, 1, block, device=dev, dtype=torch.float32)
        self.y = torch.empty(B, 1, block, device=dev, dtype=torch.float32)
        self.pre = torch.empty(B, 1, block, device=dev, dtype=torch.float32)
        self.err = torch.zeros(1, device=dev, dtype=torch.int32)
        if not (model.hidden is not None and model.hidden.shape[1] == B and dl.buffer.shape[0] == B):
            if warm:                                        # DiffDelRNN._predict_start: one stream warmed, broadcast to B
                model.initialize_hidden(1, model.max_delay)
                model.warm_start()
            else:
                model.initialize_hidden(B, model.max_delay)
        D = self.D = int(dl.max_delay)
        if dl.buffer.shape[2] != D:
            raise RuntimeError(f"BlockStreamer: delay buffer {list(dl.buffer.shape)} vs max_delay {D}")
        if model.hidden is None:
            self.h = torch.zeros(1, B, H, device=dev, dtype=torch.float32)
        else:
            self.h = model.hidden.to(device=dev, dtype=torch.float32).expand(1, B, H).contiguous().clone()
        buf = dl.buffer.to(device=dev, dtype=torch.float32).expand(B, 1, D).contiguous().clone()
        g, lib = model.GRU, _lib.lib()
        w = (ptr(g.weight_ih_l0), ptr(g.weight_hh_l0), ptr(g.bias_ih_l0), ptr(g.bias_hh_l0), ptr(model.output.weight))
        self.one_launch = H == 64
        if self.one_launch:
            C = self.C = int(lib.ntm_diffdel_stream_ring_floats(D, block))
            self.buf = torch.zeros(B, C, device=dev, dtype=torch.float32)      # the ring
            self.pos = torch.zeros(B, device=dev, dtype=torch.int64)

            def seed():
                _lib.check(lib.ntm_diffdel_stream_seed(ptr(buf), ptr(self.buf), ptr(self.pos), B, D, C, _lib.current_stream()),
                           "ntm_diffdel_stream_seed")

            def launch(warmup=0):
                rc = lib.ntm_diffdel_stream_block(*w, ptr(self.x), ptr(self.d), ptr(self.y), ptr(self.pre), B, block, block, block,
                                                  block, ptr(self.h), ptr(self.buf), C, ptr(self.pos), D, warmup, ptr(self.err),
                                                  _lib.current_stream())
                _lib.check(rc, "ntm_diffdel_stream_block")
            seed()
        else:
            self.buf = buf.clone()                          # the reference's shifted buffer, moved on in place

            def seed():
                self.buf.copy_(buf)

            def launch(warmup=0):
                rc = lib.ntm_diffdel_gru_forward_ex(*w, H, ptr(self.x), ptr(self.d), ptr(self.y), ptr(self.pre), B, block, ptr(self.h),
                                                    ptr(self.buf), D, warmup, ptr(self.err), _lib.NTM_DIFFDEL_TWO_PASS,
                                                    _lib.current_stream())
                _lib.check(rc, "ntm_diffdel_gru_forward")
        self._launch = launch
        if use_graph:                                       # the normal block; a warm-up call takes the plain launch
            h0 = self.h.clone()
            self._capture(dev, launch, lambda: (self.h.copy_(h0), seed(), self.err.zero_()))

    @torch.no_grad()
    def process(self, x_block, d_block=None, warmup=False):
        if not self.diffdel:
            if d_block is not None or warmup:
                raise TypeError("BlockStreamer.process: an RNN streamer takes x_block alone")
        else:
            if d_block is None:
                raise TypeError("BlockStreamer.process: a DiffDelRNN streamer needs d_block (B,1,block), the delays in samples")
            if tuple(d_block.shape) not in ((self.B, 1, self.block), (self.B, self.block)):
                raise ValueError(f"BlockStreamer.process: d_block {tuple(d_block.shape)}, expected {(self.B, 1, self.block)}")
            self.d.copy_(d_block.reshape(self.B, 1, self.block), non_blocking=True)
        self.x.copy_(x_block.reshape(self.B, 1, self.block), non_blocking=True)
        if warmup:
            self._launch(1)
        elif self.graph is not None:
            self.graph.replay()
        else:
            self._launch()
        return self.y

    def raise_if_violated(self):
        """The model's `assert max_delay >= max(dt)` for every block since the last check (one host synchronisation)."""
        if self.diffdel and int(self.err.item()) != 0:
            self.err.zero_()
            raise AssertionError("max_delay >= max(dt) violated")

    @torch.no_grad()
    def export_state(self):
        """-> (hidden (1,B,H), buffer (B,1,D)) in the reference's layout: what a DiffDelRNN carries after the same calls, and
        takes back (model.hidden, model.diffdel.buffer)."""
        from . import _lib
        from ._lib import ptr
        if not self.diffdel:
            raise TypeError("BlockStreamer.export_state: a DiffDelRNN streamer's state; an RNN streamer's is `h`")
        if not self.one_launch:
            return self.h.clone(), self.buf.clone()
        buf = torch.empty(self.B, 1, self.D, device=self.buf.device, dtype=torch.float32)
        rc = _lib.lib().ntm_diffdel_stream_export(ptr(self.buf), ptr(self.pos), ptr(buf), self.B, self.D, self.C, _lib.current_stream())
        _lib.check(rc, "ntm_diffdel_stream_export")
        return self.h.clone(), buf
