"""fcn8s_tensorflow_amd/fda.py on the CPU: `transfer_numpy(float64)` -- the matrix formulation, no FFT -- against tests/golden/fda_cases.npz, which
tests/golden/make_fda_cases.py wrote by the published fft2 / fftshift / window / ifft2 route; the half-width rule against hand values; the window
properties on the float64 result (inside the window the target's amplitude and the source's phase, outside it the source's spectrum); the
equal-bytes identity; every refusal."""
import functools
import os

import numpy as np
import pytest

from fcn8s_tensorflow_amd import fda as FDA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fda_cases.npz")


@functools.lru_cache(maxsize=None)
def golden():
    """The fixture's cases as dicts: name, images [N,H,W,3], targets [M,H,W,3], b, pair [N], y float64 [N,H,W,3], N, M, H, W."""
    with np.load(GOLDEN) as z:
        cases = []
        for i, name in enumerate(z["names"]):
            c = dict(name=str(name), images=z["c%d_images" % i], targets=z["c%d_targets" % i], b=int(z["c%d_b" % i]),
                     pair=z["c%d_pair" % i].astype(np.int64), y=z["c%d_y" % i])
            c["N"], c["H"], c["W"] = c["images"].shape[:3]
            c["M"] = c["targets"].shape[0]
            cases.append(c)
    return cases


def case_ids():
    return [c["name"].replace(" ", "_") for c in golden()]


def pick(name):
    return [c for c in golden() if c["name"].startswith(name)][0]


@functools.lru_cache(maxsize=None)
def restated32(i):
    """(y of transfer_numpy(float32), E = its largest distance from the fixture) of case i: the float32 restatement's own rounding."""
    c = golden()[i]
    y = FDA.transfer_numpy(c["images"], c["targets"], c["b"], c["pair"], dtype=np.float32)
    return y, float(np.abs(y.astype(np.float64) - c["y"]).max())


def test_the_fixture_holds_the_cases_of_its_description_and_stays_small():
    names = [c["name"] for c in golden()]
    assert names == ["2x2 b=0", "3x5 b=0", "3x5 b=1", "7x16 b=0", "7x16 b=1", "7x16 b=3", "8x63 b=0", "8x63 b=1", "8x63 b=3", "33x129 b=0",
                     "33x129 b=1", "33x129 b=16", "batch 3+2 16x24 b=2"]
    assert golden()[-1]["pair"].tolist() == [1, 0, 1]
    assert os.path.getsize(GOLDEN) < 480 * 1000
    for c in golden():
        assert c["y"].dtype == np.float64 and c["y"].shape == c["images"].shape and 2 * c["b"] + 1 <= min(c["H"], c["W"])


@pytest.mark.parametrize("i", range(13), ids=lambda i: "case%d" % i)
def test_the_matrix_formulation_equals_the_published_route(i):
    c = golden()[i]
    y = FDA.transfer_numpy(c["images"], c["targets"], c["b"], c["pair"])
    assert y.dtype == np.float64 and np.abs(y - c["y"]).max() < 1e-9, (c["name"], np.abs(y - c["y"]).max())
    y32, E = restated32(i)
    assert y32.dtype == np.float32 and E < 8e-4, (c["name"], E)                # float32: between 0 and 8e-4 on the 0..255 scale


def test_half_width():
    assert FDA.half_width(512, 1024, 0.01) == 5 and FDA.half_width(1024, 512, 0.09) == 46 and FDA.half_width(1024, 2048, 0.09) == 92
    assert FDA.half_width(64, 96, 0.05) == 3 and FDA.half_width(100, 100, 0.01) == 1 and FDA.half_width(99, 200, 0.01) == 0
    assert FDA.half_width(1, 7, 0.09) == 0 and isinstance(FDA.half_width(33, 129, 0.09), int) and FDA.half_width(33, 129, 0.09) == 2


@pytest.mark.parametrize("name", ["7x16 b=3", "8x63 b=1", "33x129 b=16", "batch"])
def test_the_window_takes_the_targets_amplitude_and_keeps_the_sources_phase(name):
    c = pick(name)
    b, H, W = c["b"], c["H"], c["W"]
    y = FDA.transfer_numpy(c["images"], c["targets"], b, c["pair"])
    fu, fv = np.fft.fftfreq(H, 1.0 / H).round().astype(int), np.fft.fftfreq(W, 1.0 / W).round().astype(int)
    inside = (np.abs(fu)[:, None] <= b) & (np.abs(fv)[None, :] <= b)
    assert inside.sum() == (2 * b + 1) ** 2
    for n in range(c["N"]):
        Fy = np.fft.fft2(y[n], axes=(0, 1))
        Fs = np.fft.fft2(c["images"][n].astype(np.float64), axes=(0, 1))
        Ft = np.fft.fft2(c["targets"][c["pair"][n]].astype(np.float64), axes=(0, 1))
        tol = 1e-9 * H * W
        assert np.abs(np.abs(Fy) - np.abs(Ft))[inside].max() < tol             # the amplitude inside the window is the target's
        assert np.abs(Fy - Fs / np.abs(Fs) * np.abs(Ft))[inside].max() < tol   # with the source's phase (fixture: A_s >= 1e-3 H W)
        assert np.abs(Fy - Fs)[~inside].max() < tol                            # everything outside is the source's


def test_equal_source_and_target_give_the_source_back_exactly():
    for c in (pick("33x129 b=16"), pick("batch"), pick("8x63 b=3")):
        for dtype in (np.float64, np.float32):
            y = FDA.transfer_numpy(c["images"], c["images"].copy(), c["b"], dtype=dtype)
            assert y.dtype == dtype and (y == c["images"]).all()
            assert (FDA.to_uint8(y) == c["images"]).all()
    c = pick("batch")                                                           # one of three sources has its own bytes as target
    trg = np.stack([c["targets"][0], c["images"][1]])
    y = FDA.transfer_numpy(c["images"], trg, c["b"], [0, 1, 0])
    assert (y[1] == c["images"][1]).all() and (y[0] != c["images"][0]).any()


def test_pair_none_is_n_mod_m_and_a_constant_source_stays_finite():
    c = pick("batch")
    assert (FDA.transfer_numpy(c["images"], c["targets"], c["b"]) == FDA.transfer_numpy(c["images"], c["targets"], c["b"], [0, 1, 0])).all()
    flat = np.full((1, 9, 11, 3), 77, np.uint8)
    assert np.isfinite(FDA.transfer_numpy(flat, c["targets"][:1, :9, :11], 2)).all()
    assert np.isfinite(FDA.transfer_numpy(np.zeros_like(flat), c["targets"][:1, :9, :11], 2, dtype=np.float32)).all()


def test_every_refusal():
    c = pick("batch")
    img, trg, b = c["images"], c["targets"], c["b"]
    bad = [lambda: FDA.transfer_numpy(img.astype(np.float32), trg, b), lambda: FDA.transfer_numpy(img, trg.astype(np.int32), b),
           lambda: FDA.transfer_numpy(img[0], trg, b), lambda: FDA.transfer_numpy(img[..., :2], trg[..., :2], b),
           lambda: FDA.transfer_numpy(img[:0], trg, b), lambda: FDA.transfer_numpy(img, trg[:, :15], b), lambda: FDA.transfer_numpy(img, trg[:, :, :23], b),
           lambda: FDA.transfer_numpy(img, trg, -1), lambda: FDA.transfer_numpy(img, trg, 8), lambda: FDA.transfer_numpy(img, trg, 2.0),
           lambda: FDA.transfer_numpy(img, trg, True), lambda: FDA.transfer_numpy(np.zeros((1, 200, 200, 3), np.uint8), np.zeros((1, 200, 200, 3), np.uint8), 97),
           lambda: FDA.transfer_numpy(img, trg, b, [0, 1]), lambda: FDA.transfer_numpy(img, trg, b, [0, 1, 2]), lambda: FDA.transfer_numpy(img, trg, b, [0, -1, 1]),
           lambda: FDA.transfer_numpy(img, trg, b, [0.0, 1.0, 0.0]), lambda: FDA.transfer_numpy(img, trg, b, dtype=np.float16),
           lambda: FDA.transfer_numpy(np.zeros((257, 1, 1, 3), np.uint8), np.zeros((1, 1, 1, 3), np.uint8), 0),
           lambda: FDA.validate(0.0), lambda: FDA.validate(-0.01), lambda: FDA.validate(0.1), lambda: FDA.validate("0.01"), lambda: FDA.validate(True),
           lambda: FDA.validate(float("nan")), lambda: FDA.validate(0.01, has_generator=False)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail("refusal %d did not raise" % k)
    assert FDA.validate(None) is None and FDA.validate(None, has_generator=False) is None and FDA.validate(0.09) == 0.09 and FDA.validate(0.01) == 0.01
    assert FDA.transfer_numpy(img, trg, 7).shape == img.shape                  # 2 b + 1 = 15 <= 16: the largest that fits
