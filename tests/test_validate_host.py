"""The normalised median test on the CPU: the library's host statement of the rule (`validate_velocities_host`,
csrc/validate.h) against the numpy restatement (tests/validate_restatement.py), bit for bit over the whole catalogue
(tests/validate_cases.py); what each case knows about its own answer, asserted on the restatement; the planted-outlier case;
`validation_lattice`; the refusals.  No GPU."""
import numpy as np
import pytest

import validate_cases as VC
from iceberg_tracking_code_amd import _lib, validate_velocities_host, validation_lattice
from iceberg_tracking_code_amd.validate import validate_options, validation_array
from validate_restatement import restate, same_bits

CASES = VC.catalogue()


@pytest.fixture(scope="module")
def restated():
    out = {}
    for c in CASES:
        args, kw = VC.call_args(c)
        out[c["name"]] = restate(*args, **kw)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_knows_its_answer(case, restated):
    """on the restatement, never on the code under test"""
    r, info = restated[case["name"]], case["info"]
    status = r["status"]
    for p in info.get("rejected", []):
        assert status[p] == 1, p
    if info.get("exact_rejected"):
        assert np.flatnonzero(status == 1).tolist() == info["rejected"]
    if info.get("no_status2"):
        assert not (status == 2).any()
    for p in info.get("status2", []):
        assert status[p] == 2 and np.isnan(r["r2"][p]), p
    for p in info.get("status3", []):
        assert status[p] == 3 and np.isnan(r["r2"][p]), p
    for p in info.get("judged", []):
        assert status[p] in (0, 1), p
    for p in info.get("nan_r2_kept", []):
        assert status[p] == 0 and np.isnan(r["r2"][p]), p
    for p, want in info.get("r2_exact", {}).items():
        assert r["r2"][p] == want and status[p] == 0
    if "pool_sizes" in info:
        assert sorted(r["pool_n"][r["pool_n"] > 0].tolist()) == sorted(info["pool_sizes"])
    if "largest_pool" in info:
        assert r["pool_n"].max() == info["largest_pool"] == r["pool_n"][0, 1, 1]
    assert np.array_equal(r["keep"], status != 1)


def test_catalogue_covers_what_it_claims(restated):
    sizes = np.concatenate([r["pool_n"].ravel() for r in restated.values()])
    assert {1, 2, 3, 8, 9, VC.POOL_LDS_TERMS, VC.POOL_LDS_TERMS + 1} <= set(sizes.tolist())
    seen = np.concatenate([r["status"] for r in restated.values()])
    assert set(seen.tolist()) == {0, 1, 2, 3}
    assert all(len(c["x"]) <= 400 for c in CASES if not c["name"].startswith(("lds_limit", "planted")))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_host_equals_restatement(case, restated):
    args, kw = VC.call_args(case)
    got = validate_velocities_host(*args, **kw)
    assert same_bits(got, restated[case["name"]]) is None


def test_inputs_are_not_written():
    case = CASES[-1]
    args, kw = VC.call_args(case)
    before = [a.copy() for a in args[:4]]
    validate_velocities_host(*args, **kw)
    assert all(np.array_equal(a, b) for a, b in zip(args[:4], before))


def test_validation_lattice():
    fjord = dict(x=np.array([10.0, 250.0, 130.0]), y=np.array([-40.0, 20.0, 95.0]))
    assert validation_lattice(fjord, 50.0) == dict(left=10.0, top=95.0, side=50.0, cols=5, rows=3)
    assert validation_lattice(fjord, 240.0) == dict(left=10.0, top=95.0, side=240.0, cols=1, rows=1)
    assert validation_lattice(dict(x=[3.0, 3.0], y=[1.0, 1.0]), 7.0) == dict(left=3.0, top=1.0, side=7.0, cols=1, rows=1)
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            validation_lattice(fjord, bad)


def test_validate_options():
    assert validate_options(None, 150) is None
    assert validate_options(True, 150) == dict(threshold=2.0, eps=0.01, min_neighbours=8, side=300.0)
    assert validate_options(dict(eps=0.05, side=80), 150) == dict(threshold=2.0, eps=0.05, min_neighbours=8, side=80)
    with pytest.raises(ValueError):
        validate_options(dict(treshold=1.0), 150)
    a = validation_array(validate_options(True, 150))
    assert a.dtype == np.float64 and a.tolist() == [2.0, 0.01, 8.0, 300.0]


ERRORS = dict(arg=ValueError, cap=_lib.IcelkError)


@pytest.mark.parametrize("change,kind", VC.REFUSALS, ids=VC.REFUSAL_IDS)
def test_host_refusals(change, kind):
    with pytest.raises(ERRORS[kind]):
        VC.refused_call(validate_velocities_host, change)


def test_host_refuses_groups_beyond_31_bits_and_mismatched_lengths():
    case = CASES[1]
    args, _ = VC.call_args(case)
    n = len(args[0])
    with pytest.raises(_lib.IcelkError):                                  # 49 cells x 2^26 groups = 2^31 + ...
        validate_velocities_host(*args, groups=(np.zeros(n, np.int32), 1 << 26))
    with pytest.raises(ValueError):
        validate_velocities_host(*args, groups=(np.zeros(n, np.int32), 0))
    with pytest.raises(ValueError):
        validate_velocities_host(args[0][:-1], *args[1:])
    with pytest.raises(ValueError):
        validate_velocities_host(*args, groups=(np.zeros(n - 1, np.int32), 1))
