"""A directory sweep leaves the frozen state it found (sweeps.frozen), on the device: `evaluate_cityscapes` of a frozen model keeps it frozen
and returns, key for key, the dict of an unfrozen model's call."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests.test_panoptic_facade_gpu import _same, make_image, make_model  # noqa: E402


def test_evaluate_cityscapes_keeps_a_frozen_model_frozen(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(11)
    (tmp_path / "leftImg8bit" / "aachen").mkdir(parents=True); (tmp_path / "gtFine" / "aachen").mkdir(parents=True)
    Image.fromarray(make_image(rng, 64, 96)).save(tmp_path / "leftImg8bit" / "aachen" / "aachen_000000_000019_leftImg8bit.png")
    gt = np.kron(rng.integers(0, 34, (8, 12)), np.ones((8, 8), np.int64)).astype(np.uint8)
    Image.fromarray(gt).save(tmp_path / "gtFine" / "aachen" / "aachen_000000_000019_gtFine_labelIds.png")
    images_dir, search = str(tmp_path / "leftImg8bit"), str(tmp_path / "gtFine" / "*" / "*_gtFine_labelIds.png")
    m = make_model()
    try:
        assert m.engine.get_option("frozen") == 0
        unfrozen = m.evaluate_cityscapes(images_dir, search, instance_level=False)
        assert m.engine.get_option("frozen") == 0
        m.engine.freeze(True)
        frozen = m.evaluate_cityscapes(images_dir, search, instance_level=False)
        assert m.engine.get_option("frozen") == 1
        _same(frozen, unfrozen)
        assert int(frozen["confMatrix"].sum()) == frozen["nbPixels"] == 64 * 96
    finally:
        m.close()
