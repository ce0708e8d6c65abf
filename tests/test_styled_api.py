"""The host side of the device Styled-MNIST generator (src.utils.data_utils, cvhip.styled): every bad argument is
refused before the device is touched, and the two host helpers keep the reference's contracts (no GPU)."""

import numpy as np
import pytest
import torch

import styled_ref as SR
from cvhip import styled
from src.utils import data_utils as DU

IMGS = np.zeros((4, 28, 28), dtype=np.uint8)
LABELS = [0, 1, 2, 3]
# a device that does not exist: reaching it would raise something other than the ValueError under test
NOWHERE = "cuda:63"


def test_style_names():
    assert DU.STYLE_NAMES == ("identity", "stripe", "zigzag", "canny_edges", "scale", "brightness")
    assert [styled.KINDS[s] for s in DU.STYLE_NAMES] == list(range(6))
    assert DU.parse_style("scale") == ("scale", 3) and DU.parse_style("brightness") == ("brightness", 5)
    assert DU.parse_style(("scale", 5)) == ("scale", 5) and DU.parse_style("zigzag") == ("zigzag", 1)


@pytest.mark.parametrize("styles,kw,what", [
    ({"identity": 0.5, "inverse": 0.5}, {}, "unknown style"),
    (["identity", "rotate"], {"style_dict": {c: {"train": [0]} for c in range(4)}, "split": "train"},
     "unknown style"),
    ({("scale", 0): 1.0}, {}, "severity"),
    ({("brightness", 6): 1.0}, {}, "severity"),
    ({("scale", 2.5): 1.0}, {}, "severity"),
    (["identity", "stripe"], {"style_dict": {c: {"train": [0]} for c in range(4)}}, "split"),
    (["identity", "stripe"], {"split": "train"}, "style_dict"),
    (["identity", "stripe"], {"style_dict": {c: {"train": [0]} for c in range(4)}, "split": "val"}, "split"),
    (["identity", "stripe"], {"style_dict": {c: {"train": [2]} for c in range(4)}, "split": "train"}, "indices"),
    (["identity", "stripe"], {"style_dict": {c: {"train": [0]} for c in range(3)}, "split": "train"}, "no entry"),
    ({"identity": 0.5, "stripe": 0.4}, {}, "sum to 1"),
    ({"identity": 1.5, "stripe": -0.5}, {}, "sum to 1"),
], ids=["name", "name-in-list", "sev0", "sev6", "sev-float", "k-no-split", "k-no-dict", "k-bad-split", "k-bad-index",
        "k-missing-class", "p-sum", "p-negative"])
def test_bad_styles_raise_on_the_host(styles, kw, what):
    with pytest.raises(ValueError, match=what):
        DU.DeviceStyledMNIST(IMGS, LABELS, styles, device=NOWHERE, **kw)


@pytest.mark.parametrize("images", [np.zeros((4, 28, 28), dtype=np.float32), np.zeros((4, 32, 32), dtype=np.uint8),
                                    np.zeros((4, 28, 28, 1), dtype=np.uint8), np.zeros((28, 28), dtype=np.uint8),
                                    torch.zeros(4, 28, 28, dtype=torch.int16)],
                         ids=["float", "32x32", "hwc", "one-image", "int16"])
def test_bad_images_raise_on_the_host(images):
    with pytest.raises(ValueError, match=r"uint8 \[N, 28, 28\]"):
        DU.DeviceStyledMNIST(images, LABELS, {"identity": 1.0}, device=NOWHERE)


def test_label_count_and_missing_labels():
    with pytest.raises(ValueError, match="one label per image"):
        DU.DeviceStyledMNIST(IMGS, [0, 1], {"identity": 1.0}, device=NOWHERE)
    with pytest.raises(ValueError, match="labels are required"):
        DU.DeviceStyledMNIST(IMGS, None, {"identity": 1.0}, device=NOWHERE)


def test_stylize_refuses_cpu_tensors():
    x = torch.zeros(2, 28, 28, dtype=torch.uint8)
    y = torch.zeros(2, dtype=torch.int64)
    tab = torch.ones(1, 1)
    with pytest.raises(RuntimeError, match="ROCm device"):
        styled.stylize(x, y, tab, ["identity"], [1])
    with pytest.raises(ValueError, match="unknown style"):
        styled.check_kinds(["sepia"], [1])
    with pytest.raises(ValueError, match="severity"):
        styled.check_kinds(["scale"], [9])
    assert styled.check_kinds(["canny_edges", "brightness"], [0, 2]) == ([3, 5], [0, 2])


def test_zigzag_table_matches_the_restatement():
    pts, cols = styled.zigzag_table()
    assert pts.shape == (10, 8, 2) and cols.shape == (10, 7, 2) and cols.dtype == np.int32
    for k, dr in enumerate(range(-5, 5)):
        cs, rs = SR.zigzag_polyline(0, dr)
        assert np.allclose(pts[k, :, 0], cs, rtol=0, atol=1e-12) and np.allclose(pts[k, :, 1], rs, rtol=0, atol=1e-12)
        assert np.array_equal(cols[k, :, 0], np.floor(cs[:-1])) and np.array_equal(cols[k, :, 1], np.ceil(cs[1:]))
    assert cols.min() >= 2 and cols.max() <= 28


def test_random_style_distribution():
    np.random.seed(3)
    d = DU.random_style_distribution()
    assert list(d) == ["identity", "stripe", "zigzag", "canny_edges"]
    assert abs(sum(d.values()) - 1.0) < 1e-12 and min(d.values()) > 0
    np.random.seed(3)
    assert np.array_equal(list(d.values()), np.random.dirichlet([10] * 4))
    specs = ["identity", ("scale", 5), "brightness"]
    d = DU.random_style_distribution(specs)
    assert list(d) == specs and abs(sum(d.values()) - 1.0) < 1e-12


def test_generate_style_dict():
    np.random.seed(4)
    styles = list(range(6))
    d = DU.generate_style_dict(range(10), styles, 2)
    assert sorted(d) == list(range(10))
    for c in range(10):
        tr, te = list(d[c]["train"]), list(d[c]["test"])
        assert len(tr) == 2 and len(set(tr)) == 2 and len(te) == 4
        assert sorted(tr + te) == styles and te == sorted(te)
    assert len({tuple(sorted(d[c]["train"])) for c in range(10)}) > 1
    for k in (0, 6, 7, -1):
        with pytest.raises(ValueError, match="k must be in"):
            DU.generate_style_dict(range(10), styles, k)
