"""neural-tape-modeling_amd -- MI355X-native engine for the tape-nonlinearity forward path of
01tot10/neural-tape-modeling (GRU-HS[64], DiffDelGRU-HS[64], TCN contrast point).

The directory name contains a hyphen, so import it through the root-level shim:  `import ntm_amd`.
Layout:  csrc/ (HIP kernels + C ABI -> libntm.so), model.py (reference object protocol),
epoch.py (the reference's TBPTT epoch, validation and predict-segment loops, once for single models and Replicas), utilities.py (name parsers), weights.py (exported checkpoints), harness.py (test-model.py loss loop),
distributed.py (stream sharding + the one RCCL all-reduce), critics.py (the adversarial run's critics: MultiSpecCrit on the
spectrogram, DilatedConvDisc on the waveform), adversarial.py (the adversarial run's configurations and training loop),
evaluation.py (its validation metric bundle), diffusion.py (the diffusion generators: UNet1D and the EDM sampler),
optim.py (the optimiser step on the device: FusedAdam with the gradient clip, and the EMA), datasets_diffusion.py (the
diffusion trainers' dataset classes and the device batch feeder).
"""
from . import _lib  # noqa: F401
from ._lib import NtmError, build  # noqa: F401
from .model import (RNN, DCPreESR, DiffDelRNN, ESRLoss, MRSTFTLoss, Replicas, TimeFreqConverter, TimeVaryingDelayLine, ValLossSupervised,  # noqa: F401
                    esr_dcpre_sums, esr_per_segment, esr_sums, mel_sums, spec_sums, stft_sums)
from .tape import Tape, TapeMagnetization  # noqa: F401
from .tcn import TCN  # noqa: F401
from .utilities import nextpow2, parse_hidden_size, parse_loss, parse_model  # noqa: F401
from . import adversarial, critics, datasets_diffusion, diffusion, distributed, epoch, evaluation, feeder, harness, optim, weights  # noqa: F401
from .diffusion import DiffusionGenerator, EDMTrainer, UNet1D, load_config  # noqa: F401
from .optim import FusedAdam, ema_update_  # noqa: F401

__all__ = ["RNN", "DiffDelRNN", "Replicas", "TimeVaryingDelayLine", "TCN", "Tape", "TapeMagnetization", "ESRLoss", "DCPreESR", "MRSTFTLoss", "ValLossSupervised", "TimeFreqConverter", "stft_sums", "spec_sums", "mel_sums", "esr_dcpre_sums", "esr_sums", "esr_per_segment",
           "parse_hidden_size", "parse_model", "parse_loss", "nextpow2", "weights", "critics", "adversarial", "evaluation", "build", "NtmError",
           "diffusion", "UNet1D", "DiffusionGenerator", "EDMTrainer", "load_config", "optim", "FusedAdam", "ema_update_"]
