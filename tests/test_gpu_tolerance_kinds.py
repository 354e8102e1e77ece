"""GPU test (-m gpu) of the tolerance runs one after another on one System (csrc/tolerance_mc.hip): the plain run, the run with
contributors, the run with quantiles and the Sobol run share one plan -- the tables, the round's workspace, the host forms' buffers
-- so a run meets whatever the kinds before it left there.  Every host-form call of the sequence below has to give the bytes the
same call gives on a System that has run nothing else.

samples = 600 with chunk = 256: two full rounds and a tail of 88 samples, the smallest shape with a partial round behind a full one.
Bar: bytes, every output array."""
import numpy as np
import pytest

import mc_ref as R
from oracle import oracle as O
from test_gpu_tolerance_mc import ALL46, DISTS16, N16, POS16, SEED, X16, dists_of

pytestmark = pytest.mark.gpu

SAMPLES = 600
REC3 = ALL46[:3]
assert all(DISTS16[j][0] not in (R.CORNER,) for j in range(3))  # (the Sobol run takes no CORNER dimension)


@pytest.fixture(scope="module")
def E():
    import ezpz_amd

    if ezpz_amd.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product path has no CPU fallback")
    return ezpz_amd


def fresh(E):
    return E.System(O.stack([O.fixed(v, float(X16[v])) for v in range(N16)]), N16)


def arrays_of(res):
    """{name: bytes} of every array a result carries, its contributors' included."""
    out = {}
    for name, value in vars(res).items():
        if isinstance(value, np.ndarray):
            out[name] = value.tobytes()
        elif hasattr(value, "cov"):  # McContributors
            out.update({"contributors." + k: v.tobytes() for k, v in vars(value).items() if isinstance(v, np.ndarray)})
    return out


def steps(E):
    nom = fresh(E).measure(X16[None, :], REC3)[0]
    limits, hist = (nom - 0.03, nom + 0.04), (nom - 0.05, nom + 0.08, 8)
    d = lambda k: dists_of(E, DISTS16[:k])  # noqa: E731
    plain3 = lambda s: s.tolerance_mc(X16, POS16, dists_of(E, DISTS16), REC3, SAMPLES, seed=SEED, limits=limits, hist=hist, chunk=256,  # noqa: E731
                                      keep=True)
    return [
        ("sobol k=2 m=1", lambda s: s.tolerance_sobol(X16, POS16[:2], d(2), ALL46[:1], SAMPLES, seed=SEED, chunk=256, keep=True)),
        ("plain, no records", lambda s: s.tolerance_mc(X16, POS16[:2], d(2), ALL46[:0], SAMPLES, seed=SEED, chunk=256, keep=True)),
        ("plain m=3", plain3),
        ("quantiles m=3", lambda s: s.tolerance_mc(X16, POS16[:3], d(3), REC3, SAMPLES, seed=SEED, chunk=256, quantiles=[0.0, 0.5, 0.99])),
        ("contributors k=3", lambda s: s.tolerance_mc(X16, POS16[:3], d(3), REC3, SAMPLES, seed=SEED, chunk=256, contributors=True)),
        ("sobol k=3 m=3", lambda s: s.tolerance_sobol(X16, POS16[:3], d(3), REC3, SAMPLES, seed=SEED, chunk=512, keep=True)),
        ("plain m=3 again", plain3),
    ]


def test_the_kinds_one_after_another_are_each_kind_alone(E):
    shared = fresh(E)
    for name, call in steps(E):
        got, want = arrays_of(call(shared)), arrays_of(call(fresh(E)))
        assert got.keys() == want.keys() and len(got) >= 3, (name, sorted(got), sorted(want))
        for field in want:
            assert got[field] == want[field], (name, field)
    # (the sequence did run: the last call's totals)
    assert call(shared).samples == SAMPLES
