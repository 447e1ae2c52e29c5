"""CPU companion of tests/test_sensor_suite_gpu.py: what keeps its gate, likelihood and independence tests from being vacuous, shown for
every family of tests/sensor_families.py with the fp64 restatement alone, on support.state_batch(193, 1, 18) states (without the
device's predicts) and inputs representable in either record type -- the declared count of unusable lanes and six lanes of every kind,
the reference applying exactly the usable lanes, and enough lanes on either side of both gates: the one between two neighbours of the
reference's nis and the family's fixed threshold."""
import numpy as np
import pytest

import sensor_families as F
from support import B_IND, state_batch

B = B_IND


@pytest.mark.parametrize("dtype", [32, 64])
@pytest.mark.parametrize("fam", [F.Depth(), F.Velocity(), F.Rows(3)], ids=["depth", "velocity", "rows"])
def test_the_mixed_inputs_meet_the_conditions_of_the_gpu_tests(fam, dtype):
    n = 18
    prm, nom, rot, P, prev = state_batch(B, 1, n)
    st = (nom, rot, P, prev)
    inp = fam.mixed(st, dtype, fam.aux_cpu(B, n, nom))
    kinds = inp["kinds"]
    usable = kinds == 0
    assert (~usable).sum() == fam.UNUSABLE and all((kinds == k).sum() >= 6 for k in range(1, fam.KINDS + 1))
    assert set(np.unique(kinds)) == set(range(fam.KINDS + 1)) and np.array_equal(usable, fam.usable(inp))
    with np.errstate(all="ignore"):
        _, app, nis, dof, _ = fam.ref(st, n, inp)
        assert np.array_equal(app, usable) and np.array_equal(dof, fam.rows * usable.astype(np.int32)) and (nis[~usable] == 0).all()
        thr = F.gate_between(nis, fam.SHARE)
        between = fam.ref(st, n, inp, thr)[1]
        fixed = fam.ref(st, n, inp, fam.THR)[1]
    rej = (usable & ~between).sum()
    print(f"{fam} f{dtype}: unusable {(~usable).sum()}, rejected between two neighbours {rej}, share not applied {(~between).mean():.3f}, "
          f"fixed threshold {fam.THR}: applied {fixed.sum()} / rejected {(usable & ~fixed).sum()}")
    assert rej >= 10 and (~between).mean() <= fam.CAP
    assert (usable & ~fixed).sum() >= 10 and fixed.sum() >= fam.MIN_APPLIED
    assert not (between & ~usable).any() and not (fixed & ~usable).any()
