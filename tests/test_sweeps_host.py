"""The nine directory sweeps of FCN8s (`predict_and_save` .. `predict_and_export_instances`) over sweeps.py, on the host: a recording stub engine
on CPU tensors stands in for the GPU, the ops are the modules' NumPy restatements.  Three things are held: the route an argument set takes or
the refusal it raises (one table for `resolve_route` and for the four entry points that report a route), the engine calls per image (the work
of a sweep is these calls), and the frozen state a sweep leaves behind (the one it found)."""
import itertools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from fcn8s_tensorflow_amd import cityscapes_eval as ce, instances as ins, pseudo_label as PL, regions, sweeps, temperature as ts
from fcn8s_tensorflow_amd.fcn8s import FCN8s

SIZES = {"aachen_000000_000019": (32, 48), "bonn_000001_000019": (48, 32)}        # (H, W): a walker that mixes them up fails


def _softmax(images):
    a = np.asarray(images).astype(np.int64)
    logits = (((a @ np.array([3, 5, 7]))[..., None] * (np.arange(20) + 1)) % 13).astype(np.float32) / 4
    e = np.exp(logits - logits.max(-1, keepdims=True))
    return (e / e.sum(-1, keepdims=True)).astype(np.float32)


def _like(images, a):
    return torch.from_numpy(a) if isinstance(images, torch.Tensor) else a


class StubEngine:
    """`Engine`'s calls of the sweeps, recorded: (name, the arguments that decide what is launched)."""
    device = 'cpu'
    torch = torch

    def __init__(self, frozen=False):
        self.frozen, self.calls, self.frozen_at_call = frozen, [], []

    def _log(self, *entry):
        self.calls.append(entry)
        self.frozen_at_call.append(self.frozen)

    def freeze(self, frozen=True):
        self.frozen = bool(frozen)

    def get_option(self, key):
        assert key == "frozen"
        return int(self.frozen)

    def _images(self, images, force_device=False):
        return (torch.as_tensor(np.asarray(images)),)

    def _predict(self, name, images, argmax):
        self._log(name, bool(argmax))
        p = _softmax(images)
        return _like(images, p.argmax(-1) if argmax else p)

    def predict(self, images, argmax=True):
        return self._predict('predict', images, argmax)

    def predict_tta(self, images, scales=(1.0,), flip=False, argmax=True):
        return self._predict('predict_tta', images, argmax)

    def predict_crf(self, images, crf, scales=(1.0,), flip=False, argmax=True):
        return self._predict('predict_crf', images, argmax)

    def predict_mc(self, images, samples=20, keep_prob=0.5, sample_offset=0, argmax=True, entropy=True, mutual_information=True):
        self._log('predict_mc', samples, keep_prob, bool(argmax), bool(entropy), bool(mutual_information))
        p = _softmax(images)
        maps = [_like(images, np.full(p.shape[:3], v, np.float32)) if on else None for v, on in ((0.25, entropy), (0.05, mutual_information))]
        return _like(images, p.argmax(-1) if argmax else p), maps[0], maps[1]

    def temperature_apply(self, prob, temperature, entropy=False, out=None):
        self._log('temperature_apply', bool(entropy), out is prob)
        q, h = ts.apply_numpy(prob.numpy(), 1.0 / temperature)
        assert out is prob
        prob.copy_(torch.from_numpy(q))
        return prob, torch.from_numpy(h) if entropy else None

    def pseudo_label(self, prob, thresholds=None, out_ids=None, ignore_id=255, base=None, base_fill=None, score=None, score_max=None, labels=True,
                     tables=None):
        self._log('pseudo_label', bool(labels))
        host = lambda t: None if t is None else t.numpy()
        lab, *counted = PL.tables_numpy(prob.numpy(), host(thresholds), host(out_ids), ignore_id, host(base), base_fill, host(score), score_max)
        if tables is None:
            tables = PL.new_tables_device(prob.shape[-1], 'cpu')
        for name, t in zip(PL.TABLE_NAMES, counted):
            if tables[name] is not None:
                tables[name] += torch.from_numpy(t)
        return torch.from_numpy(lab) if labels else None, tables

    def regions_clean(self, labels, min_area, connectivity=4, rounds=1, stats=False):
        self._log('regions_clean')
        labels.copy_(torch.from_numpy(regions.clean_numpy(labels.numpy(), np.asarray(min_area), connectivity, rounds)[0]))

    def regions_label(self, labels, connectivity=4, area=True):
        self._log('regions_label')
        comp, ar = regions.components_numpy(labels.numpy(), connectivity)
        return torch.from_numpy(comp), torch.from_numpy(ar) if area else None

    def instance_pair(self, prob, labels, comp, inst=None):
        self._log('instance_pair')
        rows, bad = ins.pair_rows_numpy(prob.numpy(), labels.numpy(), inst, comp=comp.numpy())
        return rows, np.stack(bad)


def make_model(frozen=False):
    m = FCN8s.__new__(FCN8s)
    m.engine, m.num_classes, m.temperature, m.pseudo_label_thresholds = StubEngine(frozen), 20, None, None
    return m


@pytest.fixture(autouse=True)
def nll_on_the_host(monkeypatch):
    """`temperature.Fitter` counts on the device only; here its one call is the NumPy restatement."""
    def nll_host(prob, gt, lut, betas, tables=None):
        _terms, nll, n, bad = ts.nll_numpy(prob.numpy(), gt.numpy(), np.asarray(lut), betas)
        tables += torch.from_numpy(np.concatenate([nll, [n], bad]))
        return tables
    monkeypatch.setattr(ts, "nll_device", nll_host)


@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    root = tmp_path_factory.mktemp("sweeps")
    rng = np.random.default_rng(5)
    things = np.array(ce.HAS_INSTANCES_IDS)
    for nm, (h, w) in SIZES.items():
        city = nm.split("_")[0]
        for d in ("leftImg8bit", "gtFine", "wrongSize"):
            (root / d / city).mkdir(parents=True, exist_ok=True)
        gt = np.kron(rng.integers(0, 34, (h // 8, w // 8)), np.ones((8, 8), np.int64)).astype(np.uint8)
        inst = gt.astype(np.uint16)
        thing = np.isin(gt, things)
        inst[thing] = gt[thing].astype(np.uint16) * 1000 + 1
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(root / "leftImg8bit" / city / (nm + "_leftImg8bit.png"))
        Image.fromarray(gt).save(root / "gtFine" / city / (nm + "_gtFine_labelIds.png"))
        Image.fromarray(inst).save(root / "gtFine" / city / (nm + "_gtFine_instanceIds.png"))
        Image.fromarray(gt[:, :-8].copy()).save(root / "wrongSize" / city / (nm + "_gtFine_labelIds.png"))
    return dict(images=str(root / "leftImg8bit"), one_city=str(root / "leftImg8bit" / "aachen"),
                labels=str(root / "gtFine" / "*" / "*_labelIds.png"), instances=str(root / "gtFine" / "*" / "*_instanceIds.png"),
                wrong=str(root / "wrongSize" / "*" / "*_labelIds.png"))


# ---- the nine methods: name -> (call(model, scenes, out_dir, **arguments), images it walks) ---------------------------------------------------
THR = np.full(20, 0.5, np.float32)
SWEEPS = {
    'predict_and_save': (lambda m, s, out, **kw: m.predict_and_save(out, s["one_city"], {1: (255, 0, 0, 127)}, **kw), 1),
    'predict_and_export_label_ids': (lambda m, s, out, **kw: m.predict_and_export_label_ids(out, s["images"], **kw), 2),
    'evaluate_cityscapes': (lambda m, s, out, **kw: m.evaluate_cityscapes(s["images"], s["labels"], **kw), 2),
    'evaluate_reliability': (lambda m, s, out, **kw: m.evaluate_reliability(s["images"], s["labels"], **kw), 2),
    'fit_temperature': (lambda m, s, out, **kw: m.fit_temperature(s["images"], s["labels"], passes=1, **kw), 2),
    'fit_pseudo_label_thresholds': (lambda m, s, out, **kw: m.fit_pseudo_label_thresholds(s["images"], **kw), 2),
    'predict_and_export_pseudo_labels': (lambda m, s, out, **kw: m.predict_and_export_pseudo_labels(out, s["images"], thresholds=THR, **kw), 2),
    'evaluate_cityscapes_instances': (lambda m, s, out, **kw: m.evaluate_cityscapes_instances(s["images"], s["instances"], **kw), 2),
    'predict_and_export_instances': (lambda m, s, out, **kw: m.predict_and_export_instances(out, s["images"], **kw), 2),
}
OLDER = ('predict_and_save', 'predict_and_export_label_ids', 'evaluate_cityscapes', 'evaluate_reliability', 'fit_temperature')


# ---- the route table ---------------------------------------------------------------------------------------------------------------------------
NO_PASSES = "no `scales` / `flip` / `crf` passes"
NO_TEMPERATURE = "calibrating Monte-Carlo samples"
NO_GATE = "it needs `samples`"
GRID = dict(samples=(None, 3), scales=(None, (1.0,), (0.5, 1.0)), flip=(False, True), crf=(None, False, True), temperature=(None, 1.0, 2.0),
            mi_max=(None, 0.1))


def expected_route(samples=None, scales=None, flip=False, crf=None, temperature=None, mi_max=None):
    """Three rules, in the order they are reported: the Monte-Carlo route has no passes; it takes no temperature; only it has a mutual
    information to gate on.  What is not refused is 'mc' with `samples`, 'passes' with any of scales / flip / crf, else 'single'."""
    passes = scales is not None or flip or crf is True
    if samples is not None and passes:
        return NO_PASSES
    if samples is not None and temperature is not None:
        return NO_TEMPERATURE
    if mi_max is not None and samples is None:
        return NO_GATE
    return 'mc' if samples is not None else 'passes' if passes else 'single'


def cases(*names):
    return [dict(zip(names, values)) for values in itertools.product(*(GRID[n] for n in names))]


def check(route_of, kw):
    want = expected_route(**kw)
    if want in ('single', 'passes', 'mc'):
        assert route_of(**kw) == want, kw
    else:
        with pytest.raises(ValueError) as e:
            route_of(**kw)
        assert want in str(e.value), kw


def test_resolve_route_names_the_route_or_refuses():
    model = make_model()
    for kw in cases(*GRID):
        check(lambda samples, scales, flip, crf, temperature, mi_max:
              sweeps.resolve_route(model, scales, flip, crf, temperature, samples, mi_max=mi_max).name, kw)
    assert model.engine.calls == []
    with pytest.raises(ValueError, match="`temperature` must be finite"):
        sweeps.resolve_route(model, None, False, None, temperature=0.0)
    with pytest.raises(ValueError, match="`mi_max` must be finite"):
        sweeps.resolve_route(model, None, False, None, samples=3, mi_max=float('inf'))


@pytest.mark.parametrize("name, arguments", [
    ('evaluate_reliability', ('samples', 'scales', 'flip', 'crf', 'temperature')),
    ('fit_temperature', ('scales', 'flip', 'crf')),
    ('fit_pseudo_label_thresholds', tuple(GRID)),
    ('evaluate_cityscapes_instances', ('samples', 'scales', 'flip', 'crf', 'temperature'))])
def test_entry_points_share_the_route_table(scenes, tmp_path, name, arguments):
    model = make_model()
    for kw in cases(*arguments):
        check(lambda **kw: SWEEPS[name][0](model, scenes, None, **kw)["route"], kw)


def test_refusals_are_written_once():
    import fcn8s_tensorflow_amd
    text = ""
    for f in sorted(os.listdir(os.path.dirname(fcn8s_tensorflow_amd.__file__))):
        if f.endswith(".py"):
            with open(os.path.join(os.path.dirname(fcn8s_tensorflow_amd.__file__), f)) as fh:
                text += fh.read()
    for message in (NO_PASSES + ";", NO_TEMPERATURE + " needs the temperature inside each sample's softmax; \"", "Cannot find any ground truth",
                    "Cannot find any images below"):
        assert text.count(message) == 1, message
    assert "crf_mod.resolve(crf) is not None else {}" not in text


# ---- the engine calls per image ----------------------------------------------------------------------------------------------------------------
def mc(samples=1, keep_prob=1.0, entropy=False, mutual_information=False):
    return ('predict_mc', samples, keep_prob, False, entropy, mutual_information)


APPLY, APPLY_ENTROPY = ('temperature_apply', False, True), ('temperature_apply', True, True)        # (entropy, out is prob)
SINGLE, FLIP, CRF, MC, T = {}, dict(flip=True), dict(crf=True), dict(samples=3), dict(temperature=2.0)
CLEAN = dict(min_region=4)
INSTANCE_TAIL = [('pseudo_label', True), ('regions_label',), ('instance_pair',)]
INSTANCE_ROUTES = [
    (SINGLE, [mc()] + INSTANCE_TAIL), ({**SINGLE, **T}, [mc(), APPLY] + INSTANCE_TAIL), ({**FLIP, **T}, [('predict_tta', False), APPLY] + INSTANCE_TAIL),
    (MC, [mc(3, 0.5)] + INSTANCE_TAIL),
    (CLEAN, [mc(), ('pseudo_label', True), ('regions_clean',), ('regions_label',), ('instance_pair',)])]
ARGMAX_ROUTES = [
    (SINGLE, [('predict', True)]), (FLIP, [('predict_tta', True)]), (CRF, [('predict_crf', True)]),
    (CLEAN, [('predict', True), ('regions_clean',)])]           # the docstrings' "per image: ... `predict` with `scales` / `flip` / `crf` on the device"


def pseudo_label_routes(labels):
    op = ('pseudo_label', labels)
    return [(SINGLE, [mc(), op]), ({**SINGLE, **T}, [mc(), APPLY, op]), (dict(temperature=1.0), [mc(), op]), (FLIP, [('predict_tta', False), op]),
            ({**CRF, **T}, [('predict_crf', False), APPLY, op]), (MC, [mc(3, 0.5), op]),
            (dict(samples=3, keep_prob=0.75, mi_max=0.1), [mc(3, 0.75, mutual_information=True), op])]


PER_IMAGE = {
    'predict_and_save': [(SINGLE, [('predict', False)]), (FLIP, [('predict_tta', False)]), (CRF, [('predict_crf', False)]),
                         (CLEAN, [('predict', True), ('regions_clean',)])],
    'predict_and_export_label_ids': ARGMAX_ROUTES,
    'evaluate_cityscapes': ARGMAX_ROUTES,
    'evaluate_reliability': [                                   # "the prediction on the device with `argmax=False`"; one temperature_apply, in place
        (SINGLE, [mc(entropy=True)]), ({**SINGLE, **T}, [mc(entropy=True), APPLY_ENTROPY]), (dict(temperature=1.0), [mc(entropy=True)]),
        (FLIP, [('predict_tta', False)]), ({**FLIP, **T}, [('predict_tta', False), APPLY]),
        (dict(samples=3, keep_prob=0.75), [mc(3, 0.75, entropy=True, mutual_information=True)])],
    'fit_temperature': [(SINGLE, [mc()]), (FLIP, [('predict_tta', False)]), (CRF, [('predict_crf', False)])],
    'fit_pseudo_label_thresholds': pseudo_label_routes(False),  # "one `fcn8s_op_pseudo_label` call without labels"
    'predict_and_export_pseudo_labels': pseudo_label_routes(True),
    'evaluate_cityscapes_instances': INSTANCE_ROUTES,           # pseudo_label for the argmax, optional regions_clean, regions_label, instance_pair
    'predict_and_export_instances': INSTANCE_ROUTES,
}


@pytest.mark.parametrize("name", list(SWEEPS))
def test_engine_calls_per_image(scenes, tmp_path, name):
    call, images = SWEEPS[name]
    for i, (kw, per_image) in enumerate(PER_IMAGE[name]):
        model = make_model()
        call(model, scenes, str(tmp_path / str(i)), **kw)
        assert model.engine.calls == per_image * images, (name, kw)
        assert all(model.engine.frozen_at_call), (name, kw)


# ---- the frozen state ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("name", list(SWEEPS))
def test_a_sweep_leaves_the_frozen_state_it_found(scenes, tmp_path, name, frozen):
    model = make_model(frozen)
    SWEEPS[name][0](model, scenes, str(tmp_path / "out"))
    assert model.engine.frozen == frozen
    assert model.engine.calls and all(model.engine.frozen_at_call)


@pytest.mark.parametrize("frozen", [False, True])
def test_a_sweep_that_raises_leaves_the_frozen_state_it_found(scenes, tmp_path, frozen):
    model = make_model(frozen)
    with pytest.raises(ValueError, match="Image widths of .* are not equal"):           # the walker of ground-truth pairs
        model.evaluate_cityscapes(scenes["images"], scenes["wrong"], instance_level=False)
    assert model.engine.frozen == frozen and model.engine.calls
    with pytest.raises(ValueError, match="Image sizes of .* are not equal"):            # the walker of every image below a directory
        model.predict_and_export_pseudo_labels(str(tmp_path / "out"), scenes["images"], thresholds=THR, base_search=scenes["wrong"], base_fill=255)
    assert model.engine.frozen == frozen


# ---- the files -----------------------------------------------------------------------------------------------------------------------------------
def test_walkers_and_loader(scenes, tmp_path):
    paths = sweeps.image_files(scenes["images"], 'png')
    assert [os.path.basename(p)[:-len("_leftImg8bit.png")] for p in paths] == sorted(SIZES)
    gts, paired = sweeps.paired_files(scenes["images"], scenes["labels"], 'png')
    assert paired == paths and len(gts) == 2
    with pytest.raises(ValueError, match="Cannot find any images below"):
        sweeps.image_files(str(tmp_path), 'png')
    assert sweeps.image_files(str(tmp_path), 'png', allow_none=True) == []
    with pytest.raises(ValueError, match="Cannot find any ground truth images"):
        sweeps.paired_files(scenes["images"], str(tmp_path / "*.png"), 'png')
    for p, nm in zip(paths, sorted(SIZES)):
        h, w = SIZES[nm]
        image, size = sweeps.load_image(p, False, 'cpu')
        assert image.dtype == torch.uint8 and tuple(image.shape) == (1, h, w, 3) and size == (w, h)
        assert np.array_equal(image[0].numpy(), np.array(Image.open(p)))
        small, size = sweeps.load_image(p, (16, 24), 'cpu')
        assert tuple(small.shape) == (1, 16, 24, 3) and size == (w, h)
        gt = np.zeros((h, w), np.uint8)
        sweeps.check_label_map(gt, (h, w), p, "gt")
        with pytest.raises(ValueError, match="Image widths"):
            sweeps.check_label_map(gt, (h, w + 1), p, "gt")
        with pytest.raises(ValueError, match="Image heights"):
            sweeps.check_label_map(gt, (h + 1, w), p, "gt")
        with pytest.raises(ValueError, match="Unknown label with id 34"):
            sweeps.check_label_map(gt + 34, (h, w), p, "gt")
