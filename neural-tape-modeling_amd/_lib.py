"""ctypes binding of libntm.so (the C ABI in include/ntm.h).

There is deliberately no fallback of any kind: if the HIP library is missing or no HIP device is
present, calls raise.  Nothing here imports or calls oracle/.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NTM_LIB_PATH") or os.path.join(_HERE, "libntm.so")   # override: kernel A/B builds
LAB_PATH = os.environ.get("NTM_LAB_PATH") or os.path.join(_HERE, "libntm_lab.so")   # laboratory kernels + diagnostics

NTM_GRU_AUTO, NTM_GRU_MFMA, NTM_GRU_VALU, NTM_GRU_MFMA2, NTM_GRU_F16X3, NTM_GRU_MFMA3, NTM_GRU_LAT, NTM_GRU_MFMA4, NTM_GRU_BF16X3 = 0, 1, 2, 3, 4, 5, 6, 7, 8
VARIANTS = {"auto": NTM_GRU_AUTO, "mfma": NTM_GRU_MFMA, "valu": NTM_GRU_VALU, "mfma2": NTM_GRU_MFMA2,
            "f16x3": NTM_GRU_F16X3, "lat": NTM_GRU_LAT, "bf16x3": NTM_GRU_BF16X3}

_vp = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int

_SIGNATURES = {
    "ntm_abi_version": (_int, []),
    "ntm_last_error": (ctypes.c_char_p, []),
    "ntm_gru_forward": (_int, [_vp] * 6 + [_int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "ntm_gru_forward_ex": (_int, [_vp] * 6 + [_int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp]),
    "ntm_gru_forward_io": (_int, [_vp] * 6 + [_int, _int, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "ntm_gru_forward_esr": (_int, [_vp] * 6 + [_int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _vp]),
    "ntm_gru_forward_losses": (_int, [_vp] * 6 + [_int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp, ctypes.c_float, _vp, _vp]),
    "ntm_delay_forward": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp]),
    "ntm_diffdel_gru_forward": (_int, [_vp] * 5 + [_int, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _int, _int,
                                                   _vp, _vp]),
    "ntm_diffdel_gru_forward_ex": (_int, [_vp] * 5 + [_int, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _int, _int,
                                                      _vp, _int, _vp]),
    "ntm_diffdel_gru_forward_esr": (_int, [_vp] * 5 + [_int, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _i64, _vp, _vp]),
    "ntm_diffdel_gru_forward_losses": (_int, [_vp] * 5 + [_int, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _i64, _vp,
                                              ctypes.c_float, _vp, _vp]),
    "ntm_esr_sums": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _vp, _vp]),
    "ntm_esr_splits": (_int, [_i64, _i64, _i64]),
    "ntm_esr_dcpre_sums": (_int, [_vp, _vp, _i64, _i64, _i64, ctypes.c_float, _vp, _vp]),
    "ntm_spec_sums": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, ctypes.c_float, _int, _vp, _vp]),
    "ntm_stft_sums": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, ctypes.c_float, _int, _vp, _vp]),
    "ntm_mel_sums": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, ctypes.c_float, _int, _int, _vp, _vp, _vp, _vp, _vp]),
    "ntm_copy2d_async": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _int, _vp]),
    "ntm_demodulate": (_int, [_vp, _vp, _int, _i64, _vp, _int, _i64, _i64, _vp, _vp]),
    "ntm_tape_record_field": (_int, [_vp, _vp, _vp, _i64, _i64, ctypes.c_double, ctypes.c_double, _vp]),
    "ntm_tape_hmag": (_int, [_vp, _vp, _i64, _i64, _vp, ctypes.c_double, ctypes.POINTER(ctypes.c_double), _vp]),
    "ntm_resample_fir": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, _vp, _vp]),
    "ntm_fir_f64": (_int, [_vp, _vp, _i64, _i64, _vp, _int, _int, _vp]),
    "ntm_tcn_forward": (_int, [_vp, _int, _int, _int, ctypes.POINTER(_int), _vp, _vp, _i64, _i64, _vp, _vp]),
    "ntm_tcn_scratch_floats": (_i64, [_i64, _i64, _int]),
    "ntm_tcn_chunk_streams": (_i64, [_i64, _i64, _int]),
    "ntm_loss_scalars": (_int, [_vp, _i64, _i64, ctypes.c_double, _vp, _vp]),
    # training of GRU-HS[64] (additions within ABI version 9)
    "ntm_gru_train_workspace_floats": (_i64, [_i64, _i64]),
    "ntm_gru_train_forward": (_int, [_vp] * 8 + [_i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ntm_gru_train_backward": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp]),
    "ntm_gru_train_reduce": (_int, [_vp, _i64, _vp, _vp]),
    "ntm_esr_grad": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "ntm_esr_dcpre_grad": (_int, [_vp, _vp, _i64, _i64, ctypes.c_float, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "ntm_delay_backward": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _int, _int, _int, _vp]),
    # R replicas per launch (additions within ABI version 9)
    "ntm_gru_train_forward_replicas": (_int, [_vp] * 8 + [_i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ntm_gru_train_backward_replicas": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "ntm_gru_train_reduce_replicas": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "ntm_loss_sums_replicas": (_int, [_vp, _i64, _i64, _int, _vp, _vp]),
    "ntm_esr_grad_replicas": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "ntm_esr_dcpre_grad_replicas": (_int, [_vp, _vp, _i64, _i64, _i64, ctypes.c_float, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "ntm_gru_forward_replicas": (_int, [_vp] * 8 + [_i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    # DiffDelRNN block by block (additions within ABI version 9)
    "ntm_diffdel_stream_ring_floats": (_i64, [_int, _i64]),
    "ntm_diffdel_stream_seed": (_int, [_vp, _vp, _vp, _i64, _int, _i64, _vp]),
    "ntm_diffdel_stream_export": (_int, [_vp, _vp, _vp, _i64, _int, _i64, _vp]),
    "ntm_diffdel_stream_block": (_int, [_vp] * 9 + [_i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _vp, _int, _int, _vp, _vp]),
    # adjoint of the STFT sums (additions within ABI version 9)
    "ntm_stft_grad_workspace_floats": (_i64, [_i64, _i64, _i64, _int, _int]),
    "ntm_spectrogram": (_int, [_vp, _i64, _i64, _int, _int, _int, _vp, _vp]),
    "ntm_spectrogram_grad": (_int, [_vp, _vp, _i64, _i64, _int, _int, _int, _vp, _vp, _int, _vp]),
    "ntm_stft_grad": (_int, [_vp, _vp, _i64, _i64, _i64, _int, _int, _int, ctypes.c_float, _vp, _vp, _vp, _int, _vp]),
    # the hinge / mean heads of the adversarial losses (additions within ABI version 9); outs / grads: host arrays of K device
    # pointers (ptr_array), elems: host int64 array (i64_array)
    "ntm_adv_head_forward": (_int, [_vp, _vp, _int, _i64, _i64, _int, _vp, _i64, _vp, _vp]),
    "ntm_adv_head_backward": (_int, [_vp, _vp, _int, _i64, _i64, _int, _vp, _vp, _vp]),
    # the delay line with float64 delays (an addition within ABI version 9): ntm_delay_forward's arguments, d a double pointer
    "ntm_delay_forward_f64": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _int, _int, _vp, _vp]),
    # the diffusion generators (additions within ABI version 9): blk is a pointer to diffusion.BlockSpec (ntm_unet_block)
    "ntm_unet_resblock_workspace_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_forward": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "ntm_unet_resblock_save_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_wgrad_floats": (_i64, [_vp]),
    "ntm_unet_resblock_partial_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_forward_save": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "ntm_unet_resblock_backward": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ntm_unet_wgrad_reduce": (_int, [_vp, _i64, _i64, _vp, _vp]),
    "ntm_unet_resblock_tiled_save_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_tiled_workspace_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_tiled_wgrad_floats": (_i64, [_vp]),
    "ntm_unet_resblock_tiled_partial_floats": (_i64, [_i64, _vp]),
    "ntm_unet_resblock_tiled_forward_save": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "ntm_unet_resblock_tiled_backward": (_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ntm_unet_down_combine_backward": (_int, [_vp] * 5 + [_i64, _int, _i64, _int, _int, _int, _vp, _vp, _vp, _vp]),
    "ntm_unet_up_combine_backward_partials": (_i64, [_i64]),
    "ntm_unet_up_combine_backward": (_int, [_vp] * 5 + [_i64, _int, _i64, _int, _int, _int, _i64, _vp, _vp, _vp, _vp]),
    "ntm_unet_down_combine": (_int, [_vp, _vp, _vp, _vp, _i64, _int, _i64, _int, _int, _int, _vp, _vp, _vp]),
    "ntm_unet_up_combine": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _int, _i64, _int, _int, _int, _vp, _vp, _vp]),
    "ntm_unet_upsample": (_int, [_vp, _vp, _i64, _i64, _int, _int, _int, _vp, _vp]),
    "ntm_edm_pre": (_int, [_vp, _vp, ctypes.c_float, ctypes.c_float, _vp, _i64, _vp, _vp, ctypes.c_float, ctypes.c_float, _i64, _i64, _vp, _vp, _vp]),
    "ntm_edm_post": (_int, [_vp, _vp, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _i64, _vp, _vp]),
    # the whole sampler in one launch: stages is a host UnetStage array (unet_stages), stages_dev its copy on the device
    "ntm_unet_sample_workspace_floats": (_i64, [_i64, _i64]),
    "ntm_unet_sample_one_launch": (_int, [_vp, _vp, _int, _vp, _vp, _i64, _int, ctypes.c_uint64, _vp, _vp, _int, _vp, _vp, _i64,
                                          _i64, _i64, _vp, _vp, _vp]),
    # the optimiser step over a list of tensors (additions within ABI version 9): p / g / m / v / dst / src are host arrays of
    # device pointers (ptr_array), n a host int64 array (i64_array)
    "ntm_multi_partials": (_i64, [_vp, _i64]),
    "ntm_multi_sqnorm": (_int, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "ntm_multi_clip_coef": (_int, [_vp, _i64, ctypes.c_float, _vp, _vp]),
    "ntm_multi_adam": (_int, [_vp, _vp, _vp, _vp, _vp, _i64, _vp] + [ctypes.c_float] * 6 + [_vp]),
    "ntm_multi_ema": (_int, [_vp, _vp, _vp, _i64, ctypes.c_float, ctypes.c_float, _vp]),
    # the batch feeder of the diffusion trainers (additions within ABI version 9): bank, bank_len, start (a host int64 array,
    # i64_array), ...
    "ntm_segment_mean": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "ntm_segment_crop": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp]),
    "ntm_segment_decimate": (_int, [_vp, _i64, _vp, _vp, _i64, _i64, _vp, _int, _int, _int, _vp, _vp]),
}
# the three critic conv stacks (additions within ABI version 9): the spectral critics (layers: ConvLayer[n], the float is the log
# floor), the dilated stack of the time-domain critic (ConvLayerD[n]) and the strided stack of the MelGAN critic (ConvLayerS[n]; for
# both the float is the LeakyReLU slope).  g / v / bias / dg / dv / dbias: host arrays of n device pointers (ptr_array); the
# strided family's outs / gouts likewise, one tensor per layer (a gouts entry may be null): one pointer more in its backward
for _p in ("speccrit", "convstack", "sconvstack"):
    _SIGNATURES[f"ntm_{_p}_saved_floats"] = _SIGNATURES[f"ntm_{_p}_workspace_floats"] = (_i64, [_i64, _i64, _i64, _int, _vp])
    _SIGNATURES[f"ntm_{_p}_forward"] = (_int, [_vp, _i64, _i64, _i64, ctypes.c_float, _int] + [_vp] * 7)
    _SIGNATURES[f"ntm_{_p}_backward"] = (_int, [_vp, _i64, _i64, _i64, ctypes.c_float, _int] + [_vp] * (12 if _p == "sconvstack" else 11))
ADV_HEAD_MODES = {"crit": 0, "gen": 1}      # include/ntm.h NTM_ADV_HEAD_CRIT / NTM_ADV_HEAD_GEN
ADV_HEAD_MAX_K, ADV_HEAD_CHUNK = 8, 4096    # include/ntm.h NTM_ADV_HEAD_MAX_K, NTM_ADV_HEAD_CHUNK
MULTI_MAX_TENSORS, MULTI_CHUNK = 64, 2048   # include/ntm.h NTM_MULTI_MAX_TENSORS, NTM_MULTI_CHUNK


class ConvLayer(ctypes.Structure):
    """include/ntm.h ntm_conv1d_layer: Conv1d(c_in, c_out, k, groups), stride 1, dilation 1, no padding."""
    _fields_ = [("c_in", ctypes.c_int32), ("c_out", ctypes.c_int32), ("k", ctypes.c_int32), ("groups", ctypes.c_int32)]


def conv_layers(spec):
    """((c_in, c_out, k, groups), ...) -> a ConvLayer array for the ntm_speccrit entry points."""
    return (ConvLayer * len(spec))(*[ConvLayer(*map(int, s)) for s in spec])


class ConvLayerD(ctypes.Structure):
    """include/ntm.h ntm_conv1d_layer_d: Conv1d(c_in, c_out, k, groups, dilation), stride 1, no padding."""
    _fields_ = [("c_in", ctypes.c_int32), ("c_out", ctypes.c_int32), ("k", ctypes.c_int32), ("groups", ctypes.c_int32),
                ("dilation", ctypes.c_int32)]


def conv_layers_d(spec):
    """((c_in, c_out, k, groups, dilation), ...) -> a ConvLayerD array for the ntm_convstack entry points."""
    return (ConvLayerD * len(spec))(*[ConvLayerD(*map(int, s)) for s in spec])


class ConvLayerS(ctypes.Structure):
    """include/ntm.h ntm_conv1d_layer_s: Conv1d(c_in, c_out, k, groups, stride, pad), dilation 1; pad_mode 0 zeros, 1 reflect."""
    _fields_ = [("c_in", ctypes.c_int32), ("c_out", ctypes.c_int32), ("k", ctypes.c_int32), ("groups", ctypes.c_int32),
                ("stride", ctypes.c_int32), ("pad", ctypes.c_int32), ("pad_mode", ctypes.c_int32)]


def conv_layers_s(spec):
    """((c_in, c_out, k, groups, stride, pad, pad_mode), ...) -> a ConvLayerS array for the ntm_sconvstack entry points."""
    return (ConvLayerS * len(spec))(*[ConvLayerS(*map(int, s)) for s in spec])


class UnetBlock(ctypes.Structure):
    """include/ntm.h ntm_unet_block (64 bytes)."""
    _fields_ = [("c0", ctypes.c_int32), ("c1", ctypes.c_int32), ("c_out", ctypes.c_int32), ("n_layers", ctypes.c_int32),
                ("T", ctypes.c_int64), ("T0", ctypes.c_int64), ("off0", ctypes.c_int64), ("T1", ctypes.c_int64),
                ("off1", ctypes.c_int64), ("init", ctypes.c_int32), ("form", ctypes.c_int32)]


USTAGE_KINDS = {"block": 0, "down": 1, "up": 2, "final": 3}     # include/ntm.h NTM_USTAGE_*
UNET_SAMPLE_MAX_STAGES, UNET_SAMPLE_MAX_STEPS, UNET_SAMPLE_SCALARS = 64, 64, 8     # include/ntm.h NTM_UNET_SAMPLE_*
UNET_STAGE_BYTES = 168


class UnetStage(ctypes.Structure):
    """include/ntm.h ntm_unet_stage (UNET_STAGE_BYTES): one call of the network in the one-launch sampler's table."""
    _fields_ = [("kind", ctypes.c_int32), ("C", ctypes.c_int32), ("S", ctypes.c_int32), ("width", ctypes.c_int32),
                ("taps", ctypes.c_int32), ("film_off", ctypes.c_int32), ("F", ctypes.c_int64), ("pyr_T", ctypes.c_int64),
                ("blk", UnetBlock)] + [(n, ctypes.c_void_p) for n in ("a", "b", "w0", "w1", "w2", "w3", "o0", "o1")]


def unet_stages(stages):
    """A list of UnetStage -> the host array ntm_unet_sample_one_launch checks."""
    return (UnetStage * len(stages))(*stages)


def ptr_array(tensors):
    """Host array of the device pointers of `tensors`, as the ntm_speccrit entry points take their parameters (None: null)."""
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


def i64_array(values):
    """Host int64 array, as the ntm_adv_head entry points take the row lengths of their outputs."""
    return (ctypes.c_int64 * len(values))(*[int(v) for v in values])


TRAIN_GRAD_FLOATS = 12929   # include/ntm.h NTM_TRAIN_GRAD_FLOATS: w_ih | w_hh | b_ih | b_hh | w_o | b_o of GRU(1, 64) + Linear(64, 1)

# include/ntm_lab.h: libntm_lab.so (older / experimental GRU kernels, diagnostic builds) -- tests and tools only
_LAB_SIGNATURES = {
    "ntm_lab_last_error": (ctypes.c_char_p, []),
    "ntm_lab_gru_forward": (_int, [_vp] * 6 + [_int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _int, _vp]),
    "ntm_debug_gru_stamps": (_int, [_vp] * 6 + [_vp, _vp, _i64, _i64, _vp, _vp, _int, _vp]),
    "ntm_debug_transpose4": (_int, [_vp, _vp, _vp]),
    "ntm_debug_gru_ablate": (_int, [_vp] * 6 + [_vp, _vp, _i64, _i64, _vp, _int, _vp]),
    "ntm_lab_tcn_forward": (_int, [_vp, _int, _int, _int, _vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "ntm_lab_tcn_stamps": (_int, [_vp]),
    "ntm_lab_tcn_trace": (_int, [_vp]),
    "ntm_lab_tape_math": (_int, [_int, _vp, _vp, _i64, ctypes.POINTER(ctypes.c_double), _vp]),
}
LAB_TAPE_OPS = {"rcp_nr": 0, "expm1_neg": 1, "coth_gt": 2, "langevin_prime_lt1": 3, "ja_f": 4}   # include/ntm_lab.h NTM_LAB_TAPE_*
LAB_VARIANTS = ("mfma", "valu")

_lib = None
_lab = None
ABI_VERSION = 9          # include/ntm.h NTM_ABI_VERSION this binding was written against
HIDDEN_SIZES = (8, 16, 32, 64)      # sizes with a kernel of their own; every H in [1, MAX_HIDDEN] runs (include/ntm.h)
MAX_HIDDEN = 1024
NTM_DIFFDEL_AUTO, NTM_DIFFDEL_TWO_PASS, NTM_DIFFDEL_FUSED = 0, 1, 2
DIFFDEL_MODES = {"auto": NTM_DIFFDEL_AUTO, "two_pass": NTM_DIFFDEL_TWO_PASS, "fused": NTM_DIFFDEL_FUSED}


class NtmError(RuntimeError):
    """A libntm.so entry point returned a negative status."""


def build(verbose=False):
    """Compile libntm.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    subprocess.run(["make", "-C", os.path.join(_HERE, "csrc")] + ([] if verbose else ["-s"]), check=True)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NtmError(f"{LIB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}` "
                           "(there is no CPU fallback for this path)")
        handle = ctypes.CDLL(LIB_PATH)
        # the version first: a stale library (the .so files are build artefacts) lacks newer symbols, and the helpful
        # message must come before the bare AttributeError of a missing one
        try:
            ver = handle.ntm_abi_version
        except AttributeError:
            raise NtmError(f"{LIB_PATH} does not export ntm_abi_version: not a libntm.so of this tree, rebuild it") from None
        ver.restype, ver.argtypes = _SIGNATURES["ntm_abi_version"]
        if ver() != ABI_VERSION:
            raise NtmError(f"{LIB_PATH} has ABI version {ver()}, this binding needs {ABI_VERSION}: rebuild it "
                           f"(`make -C {os.path.join(_HERE, 'csrc')}`)")
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(handle, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype, fn.argtypes = res, args
        _lib = handle
    return _lib


def lab():
    """libntm_lab.so: the laboratory kernels (kernel_variant in LAB_VARIANTS) and the diagnostic entry points.  The
    product path (kernel_variant "auto" / "mfma2" / "lat" / "f16x3" / "bf16x3") never loads it."""
    global _lab
    if _lab is None:
        if not os.path.exists(LAB_PATH):
            raise NtmError(f"{LAB_PATH} is missing: build it with `make -C {os.path.join(_HERE, 'csrc')}`")
        handle = ctypes.CDLL(LAB_PATH)
        for name, (res, args) in _LAB_SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = res, args
        _lab = handle
    return _lab


def gru_forward_fn(variant_name, hidden_size=64):
    """-> (entry point with ntm_gru_forward_ex's signature, error-message getter) for a kernel_variant name."""
    if variant_name in LAB_VARIANTS and hidden_size == 64:
        return lab().ntm_lab_gru_forward, lab().ntm_lab_last_error
    return lib().ntm_gru_forward_ex, lib().ntm_last_error


def check(rc, what, last_error=None):
    if rc != 0:
        raise NtmError(f"{what} failed ({rc}): {(last_error or lib().ntm_last_error)().decode()}")


def ptr(t):
    """Device pointer of a torch tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def current_stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
