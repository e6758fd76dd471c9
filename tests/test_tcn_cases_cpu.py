"""CPU: the cases of tests/test_gpu_tcn.py are what they claim to be.  Every exact network meets the exactness condition, the
float32 C oracle reproduces the float64 reference bit for bit on it (so `==` is a fair bar for the device), every table row is
the edge its comment names, and the probe returns an inner block's activation exactly."""
import numpy as np
import pytest
import torch

import oracle
from tcn_cases import (B_EXACT, C, DENSE, EIGHTHS, FIRST, FIRST_D1, K, PG, PG_DILS, POLY, REPEAT_ROWS, assert_exact, block_kernel,
                       dense_tcn, exact_case, exact_tcn, first_mismatch, first_shape, pg_shape, poly_shape, probe, ref64, row_id,
                       unit_of, with_probe)

DEEP = [((1, 7, 3), 300), ((1, 600, 2), 1500), ((1, 10, 100, 1000), 2100)]


def oracle_forward(m, x):
    return oracle.tcn_forward(m.packed_params().numpy(), len(m.dilations), C, K, m.dilations, x[:, 0].numpy(), threads=x.shape[0])


def check_exact_and_oracle(dilations, T):
    m, x, y64, acts, bounds = exact_case(dilations, T)
    assert_exact(bounds)
    assert x.shape == (B_EXACT, 1, T) and len(acts) == len(dilations) and acts[-1].shape == (B_EXACT, T, C)
    assert float(y64.abs().max()) > 0 and float(m.out_bias) != 0
    bad = first_mismatch(torch.from_numpy(oracle_forward(m, x)), y64)
    assert bad is None, f"{dilations} T={T}: oracle float32 != float64 at (stream, sample) {bad}"


def includes(shape, edge):
    return all(shape[k] == v for k, v in edge.items())


def test_the_case_tables_are_what_their_comments_say():
    for d, T, edge in FIRST_D1 + FIRST:
        assert includes(first_shape(d, T), edge), (d, T, first_shape(d, T))
    assert {first_shape(d, T)["kernel"] for d, T, _ in FIRST_D1} == {"first_d1"} and {first_shape(d, T)["kernel"] for d, T, _ in FIRST} == {"first"}
    for d, T, edge in POLY:
        assert block_kernel(d) == "poly" and includes(poly_shape(d, T), edge), (d, T, poly_shape(d, T))
    for d, T, edge in PG:
        assert block_kernel(d) == "pg" and includes(pg_shape(d, T), edge), (d, T, pg_shape(d, T))
    # the edges the tables exist for
    assert {poly_shape(d, T)["tpp"] for d, T, _ in POLY} >= {1, 2, 3, 4, 5, 6, 7, 8, 9}
    assert any(s["wgs"] == 2 and s["starts"][1][1] != 0 for s in (poly_shape(d, T) for d, T, _ in POLY))      # a workgroup that starts mid-phase
    assert any(T < d for d, T, _ in POLY) and max(d for d, _, _ in POLY) == 511 and min(PG_DILS) == 512
    assert {pg_shape(d, T)["mtot"] for d, T, _ in PG} == {1, 2, 3, 14, 15, 17, 31, 33}
    assert {pg_shape(d, T)["niter"] for d, T, _ in PG} == {1, 2, 7, 8, 9, 16, 17}
    assert {pg_shape(d, 1)["last_group_phases"] for d in PG_DILS} == {1, 15, 16} and len(PG) == 48 and len(POLY) == 20
    for name, (d, T) in REPEAT_ROWS.items():
        table = {"first_d1": FIRST_D1, "first": FIRST, "poly": POLY, "pg": PG}[name]
        assert (d, T) in [(r[0], r[1]) for r in table] and T % 16 != 0
    assert max(T for _, T, _ in FIRST_D1 + FIRST + POLY + PG) <= 17000
    assert len(DENSE) == 6 and sum(1 for _, _, amp in DENSE if amp > 1) == 1


def test_the_mirror_against_a_count_by_hand():
    # dil 200, T 8000: 40 outputs per phase = 3 tiles of 16; 600 tiles; tile 512 = phase 170, third tile
    assert poly_shape(200, 8000) == dict(tpp=3, total=600, wgs=2, niter=[64, 11], starts=[(0, 0), (170, 2)], empty_phases=0, empty_last_tiles=0)
    # dil 513, T 1027: 33 groups of 16 phases (the last with phase 512 alone), 17 workgroups, time indices 0, 1, 2
    assert pg_shape(513, 1027) == dict(groups=33, wgs=17, idle_pair=True, last_group_phases=1, mtot=3, niter=2, zero_page_groups=0, straddles=True)


def test_exact_networks_use_every_parameter_the_kernels_index():
    m = exact_tcn((1, 7), 5)
    for l in (0, 1):
        assert sorted(m.prelu[l].tolist()) == list(EIGHTHS)                          # 32 distinct slopes per block
    W = m.conv_weight[1]
    assert set(W.unique().tolist()) == {-1.0, 0.0, 1.0} and bool(((W != 0).sum(1) == 3).all())      # 3 input channels per (co, tap)
    assert bool(((W != 0).sum((0, 2)) > 0).all()) and bool(((m.res_weight[1] != 0).sum((1, 2)) == 2).all())
    assert bool((m.out_weight != 0).all()) and float(m.out_bias) != 0 and float(m.out_bias) == round(float(m.out_bias))
    assert unit_of(m.prelu[0]) == 0.125 and unit_of(m.conv_weight[1]) == 1.0 and unit_of(torch.tensor([0.1])) == 2.0 ** -27


@pytest.mark.parametrize("d", [1, 2, 33, 600])
def test_first_block_cases_are_exact_and_the_oracle_agrees(d):
    for dd, T, _ in FIRST_D1 + FIRST:
        if dd == d:
            check_exact_and_oracle((d,), T)


@pytest.mark.parametrize("row", POLY, ids=row_id)
def test_polyphase_cases_are_exact_and_the_oracle_agrees(row):
    check_exact_and_oracle((1, row[0]), row[1])


@pytest.mark.parametrize("row", PG, ids=row_id)
def test_phase_group_cases_are_exact_and_the_oracle_agrees(row):
    check_exact_and_oracle((1, row[0]), row[1])


@pytest.mark.parametrize("dilations,T", DEEP, ids=lambda v: str(v))
def test_deep_exact_networks(dilations, T):
    check_exact_and_oracle(dilations, T)


@pytest.mark.parametrize("dilations,T", [((33,), 33), ((1, 7), 337), ((1, 513), 514)], ids=lambda v: str(v))
def test_the_probe_returns_the_inner_activation_exactly(dilations, T):
    """The probe block and the one-hot output conv add nothing but exact zeros: the oracle, run through the probe, gives the
    float64 reference's activation of the block in front of it."""
    m, x, _, acts, _ = exact_case(dilations, T)
    got = probe(m, lambda pm: oracle_forward(pm, x))
    bad = first_mismatch(got, acts[-1])
    assert got.shape == (B_EXACT, T, C) and bad is None, f"{dilations} T={T}: (stream, sample, channel) {bad}"


def test_the_probe_passes_any_finite_float():
    """... and not only integers: a dense float network's inner activation comes through the probe bit for bit (float64 here:
    the probe's own arithmetic, F.conv1d with weights 0 and 1)."""
    m = dense_tcn((2, 5), 9)
    x = torch.from_numpy(np.random.default_rng(3).uniform(-0.8, 0.8, (2, 1, 90)).astype(np.float32))
    _, acts, _ = ref64(m, x)
    pm = with_probe(m)
    with torch.no_grad():
        pm.out_weight[0, 17, 0] = 1.0
    y, pacts, _ = ref64(pm, x)
    assert torch.equal(pacts[-1], acts[-1]) and torch.equal(y, acts[-1][:, :, 17]) and torch.equal(pacts[1], acts[1])
