"""tests/bound_ref.py (the fp64 statement of cv_snn_bounds the GPU tests compare against) against the reference
notebook's own SNN / PSSNN classes, through tests/golden/mi_bounds.npz (recipe: tests/golden/gen_mi_bounds.py).  No GPU."""

import os

import numpy as np
import pytest

import bound_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mi_bounds.npz")
CASES = ("blobs", "antipodal", "antipodal_singletons", "d1", "one_label", "wide_labels", "zero_row")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_holds_every_case(golden):
    assert sorted(k[:-3] for k in golden.files if k.endswith("__x")) == sorted(CASES)
    assert golden["taus"].tolist() == [0.01, 0.1, 0.3, 1.0]
    shapes = {k: golden[k + "__x"].shape for k in CASES}
    assert shapes == {"blobs": (96, 3), "antipodal": (70, 5), "antipodal_singletons": (70, 5), "d1": (9, 1),
                      "one_label": (33, 4), "wide_labels": (40, 8), "zero_row": (24, 3)}
    for k in CASES:
        assert golden[k + "__x"].dtype == np.float32 and golden[k + "__label"].dtype == np.int64
    lab = golden["wide_labels__label"]
    assert set(lab.tolist()) == {5, 5 + 2 ** 32, 7}
    assert len(set((lab & 0xFFFFFFFF).tolist())) == 2  # they alias when truncated
    assert (golden["zero_row__x"] == 0).all(axis=1).sum() == 1


@pytest.mark.parametrize("case", CASES)
def test_bound_ref_matches_the_notebook(golden, case):
    bound, count, _ = bound_ref.bounds(golden[case + "__x"], golden[case + "__label"], golden["taus"])
    want, want_count = golden[case + "__value"], golden[case + "__count"]
    assert np.array_equal(count, want_count)
    assert np.array_equal(np.isnan(bound), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.abs(bound[ok] - want[ok]).max() <= 1e-12


def test_antipodal_case_defeats_a_fixed_shift(golden):
    """PS-SNN at tau = 0.01 is about 200 with all 70 rows finite: every negative similarity is about -1, so a kernel
    that shifts by the bound s <= 1, exp((s - 1) / tau) = exp(-200), underflows in fp32 and drops every row."""
    assert golden["taus"][0] == 0.01
    v, c = golden["antipodal__value"][0, 1], golden["antipodal__count"][0, 1]
    assert 199.0 < v < 201.0 and c == 70
    assert np.exp(np.float32(-200.0)) == 0
    # the singleton variant: the two rows without a positive are dropped from SNN alone
    assert golden["antipodal_singletons__count"][0].tolist() == [68, 70]
    # one label for all: PS-SNN has no finite row
    assert golden["one_label__count"][:, 1].tolist() == [0, 0, 0, 0] and np.isnan(golden["one_label__value"][:, 1]).all()


def test_blob_layout(golden):
    assert int(golden["blob_rows_100_3"]) == 99 and int(golden["blob_rows_96_4"]) == 96
    assert np.array_equal(golden["blob_label_100_3"], np.arange(99) // 33)
    assert np.array_equal(golden["blob_label_96_4"], np.arange(96) // 24)
