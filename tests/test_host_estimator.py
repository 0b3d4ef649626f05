"""Host-side checks of the output-feedback additions (ABI v7) that need no GPU: the
measurement noise's sampler and the ctypes mirror of ntm_estimator.
"""
import ctypes as C
import math

import numpy as np


def test_meas_sample_matches_the_oracle_generator():
    """ntm_meas_sample (the device's generator code compiled for the host) == the NumPy
    oracle's gen_normal channels 2 and 3, bit for bit; counter-based (a shard's first_id
    offset reproduces the same values); the channels are not the plant disturbance's."""
    import ntm_mpc
    from oracle import ntm_oracle as O
    for seed, first, k in ((20241220, 0, 0), (7, -5, 13), (2 ** 64 - 1, 10 ** 12, 2 ** 31 - 1)):
        g = ntm_mpc.ScenarioGen(seed=seed, first_id=first)
        lib = ntm_mpc.meas_sample(g, 300, k)
        py = np.array([[O.gen_normal(seed, first + s, k, 2), O.gen_normal(seed, first + s, k, 3)] for s in range(300)])
        np.testing.assert_array_equal(lib, py)
        shard = ntm_mpc.meas_sample(ntm_mpc.ScenarioGen(seed=seed, first_id=first + 100), 200, k)
        np.testing.assert_array_equal(shard, lib[100:])
        dist = ntm_mpc.scenario_sample(g, 300, k)[:, 2:]
        assert not np.any(lib == dist)
    big = ntm_mpc.meas_sample(ntm_mpc.ScenarioGen(seed=3), 200_000, 5)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1.0) < 0.01
    assert np.abs(big).max() <= 2 * math.sqrt(3)
    assert abs(np.corrcoef(big[:, 0], big[:, 1])[0, 1]) < 0.01
    w = ntm_mpc.scenario_sample(ntm_mpc.ScenarioGen(seed=3), 200_000, 5)[:, 2]
    assert abs(np.corrcoef(big[:, 0], w)[0, 1]) < 0.01          # independent of the plant's disturbance


def test_estimator_struct_layout_and_abi():
    """ctypes mirror of ntm_estimator: two int32, then three double pairs (56 bytes); a
    scalar option sets both components."""
    import ntm_mpc
    from ntm_mpc._lib import ABI_VERSION, NtmEstimator
    assert C.sizeof(NtmEstimator) == 56
    assert [getattr(NtmEstimator, f).offset for f in ("nominal_model", "reserved", "gain", "kappa", "sigma_y")] == \
        [0, 4, 8, 24, 40]
    e = ntm_mpc.Estimator(nominal_model=True, gain=0.5, kappa=(0.5, 0.25), sigma_y=(2.0 ** -10, 16.0)).to_c()
    assert (e.nominal_model, e.reserved) == (1, 0)
    assert list(e.gain) == [0.5, 0.5] and list(e.kappa) == [0.5, 0.25] and list(e.sigma_y) == [2.0 ** -10, 16.0]
    assert ABI_VERSION == 7 and ntm_mpc.load().ntm_abi_version() == 7
