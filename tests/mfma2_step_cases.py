"""Case table of tests/test_gpu_mfma2_step_edges.py, shared with tools/make_goldens_mfma2_bits.py (which records
tests/golden/mfma2_step_bits.npz from it): the step counts that reach every compile-time copy of gru_mfma2_kernel's step
and the inputs of the smallest batches the kernel accepts."""
import numpy as np

# T: steps 0-1 alone, the phase-2 copy (T >= 3), the two-step loop over steps 4-33, the phase-34 and phase-36 copies, the
# second loop, one whole tile and the run-time tail behind it (65-67, 129), three tiles + a ragged fourth (200)
STEP_T = (1, 2, 3, 4, 35, 36, 37, 63, 64, 65, 66, 67, 129, 200)
T_MAX = max(STEP_T)
SMALL_B = (16, 17)               # one stream group; a ragged second group
MANY_GROUPS_T = 130              # at 16 x (CUs + 1) streams: the small-LDS build (YPN = 4)
CUTS = (3, 64, 133)              # chunk lengths of the chunked run of T = 200
SEED = 20250
assert sum(CUTS) == T_MAX


def inputs(B, T=T_MAX):
    """(x (B, T), h0 (B, 64)) float32 from the fixed seed; x of a shorter T is the prefix of the longest one."""
    rng = np.random.default_rng(SEED + B)
    x = rng.uniform(-0.5, 0.5, (B, T_MAX)).astype(np.float32)
    h0 = rng.uniform(-0.3, 0.3, (B, 64)).astype(np.float32)
    return np.ascontiguousarray(x[:, :T]), h0
