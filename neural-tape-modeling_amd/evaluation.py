"""`evaluation.val_loss_supervised` of the reference (code/evaluation.py:18-126): the validation metric bundle of the adversarial
run with the running-sum protocol its training script drives -- `add_loss` per validation batch, `end_val` per epoch, `losses`
and `bst_losses` read in between.  The metrics themselves are model.ValLossSupervised's (the device kernels); this module adds
only the bookkeeping, statement for statement."""
from .model import SPEC_SCALES, ValLossSupervised

KEYS = ("ms_spec_loss", "ms_log_spec_loss", "mel_spec_loss", "log_mel_spec_loss", "ESR", "MSE", "ESRDCPre")


class val_loss_supervised(ValLossSupervised):
    """Supervised validation loss with the reference's constructor and protocol.  `device` is accepted as in the reference and
    not used: the kernels run where the tensors are (a HIP device; there is no CPU path).
      losses       the sums of the current validation pass, one entry per key (python floats);
      bst_losses   per key [step of the best mean so far, that mean], starting at [0, 1e9];
      iter_count   batches added since the last end_val.
    """

    def __init__(self, device='cpu', spec_scales=[2048, 1024, 512, 256, 128, 64]):
        super().__init__(spec_scales=spec_scales)
        self.spec_scales = spec_scales
        self.losses = {key: 0 for key in KEYS}
        self.bst_losses = {key: [0, 1e9] for key in KEYS}
        self.iter_count = 0

    def add_loss(self, output, target):
        """Add the losses of one batch ((B, T) tensors); the first call after end_val starts the sums again."""
        if self.iter_count == 0:
            self.losses = {key: 0 for key in KEYS}

        losses = self(output, target)
        for key in losses:
            self.losses[key] += losses[key]
        self.iter_count += 1

    def end_val(self, cur_step):
        """End validation: a key whose mean over the pass is below its best so far records [cur_step, mean]."""
        for key in self.losses:
            loss = self.losses[key] / self.iter_count
            if loss < self.bst_losses[key][1]:
                self.bst_losses[key] = [cur_step, loss]
        self.iter_count = 0


assert tuple(SPEC_SCALES) == (2048, 1024, 512, 256, 128, 64)      # the reference's default, restated in the signature above
