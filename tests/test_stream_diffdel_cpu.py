"""CPU: the host side of the DiffDelRNN block-streaming entry points (include/ntm.h, ntm_diffdel_stream_*): the ring length, the
empty calls and the refusals, all decided before a device is touched."""
import ntm_amd


def test_ring_length_is_the_next_power_of_two():
    L = ntm_amd._lib.lib()
    for D, block, want in [(11001, 64, 16384), (11001, 512, 16384), (256, 64, 512), (1, 1, 2), (0, 1, 1), (7, 1, 8), (7, 2, 16),
                           (1000, 24, 1024), (1000, 25, 2048), (0, 0, 1)]:
        assert L.ntm_diffdel_stream_ring_floats(D, block) == want, (D, block)
    assert L.ntm_diffdel_stream_ring_floats(-1, 64) == 0 and L.ntm_diffdel_stream_ring_floats(7, -1) == 0


def test_empty_calls_and_refusals_need_no_device():
    L = ntm_amd._lib.lib()
    one, two = 16, 32
    blk = lambda B, block, C, D=7, h=one, y=two, pre=None: L.ntm_diffdel_stream_block(            # noqa: E731
        one, one, one, one, one, one, one, y, pre, B, block, block, block, block, h, one, C, one, D, 0, None, None)
    assert blk(0, 64, 128) == 0 and blk(3, 0, 128) == 0 and blk(0, 0, 1) == 0
    assert blk(-1, 64, 128) == -1 and b"negative size" in L.ntm_last_error()
    assert blk(3, 64, 64) == -1 and b"D + block" in L.ntm_last_error()
    assert blk(3, 64, 96) == -1 and b"power of two" in L.ntm_last_error()
    assert blk(3, 64, 128, h=None) == -1 and b"null pointer" in L.ntm_last_error()
    assert blk(3, 64, 128, y=one) == -1 and b"alias" in L.ntm_last_error()
    assert blk(3, 64, 128, pre=two) == -1 and b"alias" in L.ntm_last_error()
    assert L.ntm_diffdel_stream_seed(None, None, None, 0, 7, 8, None) == 0
    assert L.ntm_diffdel_stream_export(None, None, None, 0, 7, 8, None) == 0
    assert L.ntm_diffdel_stream_seed(one, None, one, 2, 7, 8, None) == -1 and b"null pointer" in L.ntm_last_error()
    assert L.ntm_diffdel_stream_seed(one, one, one, 2, 9, 8, None) == -1 and b"power of two" in L.ntm_last_error()
    assert L.ntm_diffdel_stream_export(one, one, None, 2, 7, 8, None) == -1 and b"null pointer" in L.ntm_last_error()
