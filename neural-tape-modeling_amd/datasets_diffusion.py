"""The training data of the diffusion nets: the reference's dataset classes (code/datasets_diffusion.py) and a feeder that keeps
the whole batch path of code/train-diffusion.py (`next(dset)` + `Trainer.get_batch`) on the device.

  TapeHissdset(dset_args, overfit=False, seed=42)      the noise net's segments: files `target*.wav`, one crop per file pick
  ToyTrajectories(dset_args, overfit=False, seed=42)   the trajectory nets' segments: files `*.wav`, eight crops per file pick
  DeviceSegmentFeeder(dataset, batch, fs_out, device)  the same batches from a bank of the files on the device, two launches each

Kept from the reference: the attributes seg_len, fs, overfit, train_samples; the seeding of `random` and `np.random` in the
constructor; the file patterns, in glob.glob's order (unsorted, as there); the empty-folder and sampling-rate assertions; the
calls on the two generators, in order (picks()); the arithmetic of a segment: stereo mixed by np.mean(axis=1) of the float64
data, the crop, astype('float32'), minus np.mean of the crop.
Different: files are read with feeder.read_wav (scipy) where the reference uses soundfile -- for PCM files the same values, an
integer over a power of two -- and a file is read once and kept, mixed to mono in float32, where the reference reads the whole
file again for every pick.  Rounding the mix to float32 before the crop gives the crop's values: astype is elementwise.
"""
import glob
import math
import os
import random

import numpy as np
import torch

from . import _lib, diffusion, feeder


class _CropDataset(torch.utils.data.IterableDataset):
    PATTERN = None      # the files of the folder
    CROPS = None        # crops per file pick

    def __init__(self, dset_args, overfit=False, seed=42):
        super().__init__()
        self.seg_len = int(dset_args.seg_len)
        self.fs = dset_args.fs
        self.overfit = overfit
        random.seed(seed)
        np.random.seed(seed)
        path = dset_args.path
        orig_p = os.getcwd()
        os.chdir(path)
        try:
            filelist = glob.glob(self.PATTERN)
        finally:
            os.chdir(orig_p)
        filelist = [os.path.join(path, f) for f in filelist]
        assert len(filelist) > 0, "error in dataloading: empty or nonexistent folder"
        self.train_samples = filelist
        self._mono = {}         # path -> the file mixed to mono, float32 (host)
        self._frames = {}       # path -> its length in samples (a DeviceSegmentFeeder fills this from its bank)

    def mono(self, num):
        """File `num` of train_samples mixed to mono, float32; read at its first use."""
        file = self.train_samples[num]
        if file not in self._mono:
            data, samplerate = feeder.read_wav(file)                 # float32 (C, N): the values soundfile returns as float64
            assert samplerate == self.fs, "wrong sampling rate"
            data = np.ascontiguousarray(data.T, dtype=np.float64)
            data_clean = np.mean(data, axis=1) if data.shape[1] > 1 else data[:, 0]
            self._mono[file] = data_clean.astype('float32')
            self._frames[file] = len(data_clean)
        return self._mono[file]

    def frames(self, num):
        file = self.train_samples[num]
        if file not in self._frames:
            self.mono(num)
        return self._frames[file]

    def picks(self):
        """(file index, first sample of the crop), for ever: the reference's calls on `random` and `np.random`, in its order."""
        while True:
            num = random.randint(0, len(self.train_samples) - 1)
            n = self.frames(num)
            for _ in range(self.CROPS):
                yield num, np.random.randint(0, n - self.seg_len)

    def __iter__(self):
        for num, idx in self.picks():
            segment = self.mono(num)[idx:idx + self.seg_len].copy()
            segment -= np.mean(segment, axis=-1)
            yield segment


class TapeHissdset(_CropDataset):
    PATTERN, CROPS = "target*.wav", 1


class ToyTrajectories(_CropDataset):
    PATTERN, CROPS = "*.wav", 8


class DeviceSegmentFeeder:
    """Batches of a TapeHissdset / ToyTrajectories as `next(dset)` + `Trainer.get_batch()` of code/train-diffusion.py deliver them --
    (batch, ceil(new seg_len / orig)) float32 on the device, orig : new the reduced ratio dataset.fs : fs_out -- without the host
    in the path.  The files live on the device once, as a bank: each read with feeder.read_wav_device, stereo mixed once in
    float64 and rounded to float32 (exact for 16-bit PCM), concatenated; the host keeps the offsets.  next_batch() draws `batch`
    picks from dataset.picks() -- the same calls on the same generators as iterating the dataset -- and runs two launches of
    csrc/segment_feed.hip: the crops' means (ntm_segment_mean), then the crop (ntm_segment_crop, equal rates) or the crop, mean
    subtraction and polyphase filter in one pass (ntm_segment_decimate, new == 1).  A reduced ratio with new > 1, which no
    configuration of the reference has, takes the crop through diffusion.apply_resample_kernel (torch).  The filter is built once,
    with diffusion.sinc_resample_kernel; torchaudio rebuilds it per call.
    The sampling rate of every file is checked when the bank is loaded; the reference checks a file when it is picked."""

    def __init__(self, dataset, batch, fs_out, device):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"DeviceSegmentFeeder: HIP device only (no CPU fallback): the device is {self.device}")
        self.dataset, self.batch, self.seg_len = dataset, int(batch), dataset.seg_len
        g = math.gcd(int(dataset.fs), int(fs_out))
        self.orig, self.new = int(dataset.fs) // g, int(fs_out) // g
        self.kernel = self.width = None
        if self.orig != self.new:
            kernel, self.width = diffusion.sinc_resample_kernel(self.orig, self.new)
            self.kernel = kernel.to(self.device)
        parts, self.offsets, total = [], [], 0
        for file in dataset.train_samples:
            x, fs = feeder.read_wav_device(file, self.device)
            assert fs == dataset.fs, "wrong sampling rate"
            parts.append(x[0] if x.shape[0] == 1 else x.double().mean(0).float())
            self.offsets.append(total)
            total += parts[-1].numel()
            dataset._frames[file] = parts[-1].numel()
        self.bank = torch.cat(parts).contiguous()
        self._picks = dataset.picks()
        self.last_picks = None
        self.out_len = int(math.ceil(self.new * self.seg_len / self.orig))

    def next_batch(self):
        self.last_picks = [next(self._picks) for _ in range(self.batch)]
        return self.rows([self.offsets[num] + int(idx) for num, idx in self.last_picks])

    def rows(self, starts):
        """The batch whose row b is the crop bank[starts[b] : starts[b] + seg_len]."""
        L, B, dev = self.seg_len, len(starts), self.device
        lib, start, stream = _lib.lib(), _lib.i64_array(starts), _lib.current_stream()
        mean = torch.empty(B, dtype=torch.float32, device=dev)
        bank, n = _lib.ptr(self.bank), self.bank.numel()
        with torch.cuda.device(dev):
            _lib.check(lib.ntm_segment_mean(bank, n, start, B, L, _lib.ptr(mean), stream), "ntm_segment_mean")
            if self.kernel is not None and self.new == 1:
                out = torch.empty(B, self.out_len, dtype=torch.float32, device=dev)
                _lib.check(lib.ntm_segment_decimate(bank, n, start, _lib.ptr(mean), B, L, _lib.ptr(self.kernel), self.orig, self.width,
                                                    self.kernel.shape[-1], _lib.ptr(out), stream), "ntm_segment_decimate")
                return out
            out = torch.empty(B, L, dtype=torch.float32, device=dev)
            _lib.check(lib.ntm_segment_crop(bank, n, start, _lib.ptr(mean), B, L, _lib.ptr(out), stream), "ntm_segment_crop")
        if self.kernel is None:
            return out
        return diffusion.apply_resample_kernel(out, self.kernel, self.orig, self.new, self.width)
