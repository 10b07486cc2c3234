"""The augmentors without a GPU: the NumPy restatement (tests/augment_cases.py) against Pillow itself, exactly; the
product's CPU path (data.augmentor) against the restatement, exactly, on every case; sample()'s draws; the operator's
Meta kernel and the argument checks that run before any launch."""
import dataclasses

import numpy as np
import pytest
import torch

import augment_cases as ac
from data.augmentor import PARAM_DOUBLES, AugmentParams, FlowAugmentor, SparseFlowAugmentor, resized_size

NAMES = [c.name for c in ac.CASES]


def _augmentor(case):
    return (SparseFlowAugmentor if case.sparse else FlowAugmentor)(case.crop)


def _run(case, device="cpu"):
    (img1, img2, flow, valid), want, _ = ac.expected(case.name)
    t = lambda a: torch.from_numpy(a.copy()).to(device)  # noqa: E731
    return _augmentor(case).augment_batch(t(img1), t(img2), t(flow), t(valid) if case.sparse else None,
                                          params=case.params), want


# ------------------------------------------------------------------------------------------- restatement vs Pillow
def _all_colours():
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8)


def _pil_convert(pixels, src_mode, dst_mode):
    Image = pytest.importorskip("PIL.Image")
    img = Image.frombytes(src_mode, (4096, 4096), pixels.tobytes())
    return np.frombuffer(img.convert(dst_mode).tobytes(), np.uint8).reshape(-1, 3)


@pytest.mark.parametrize("direction", ["rgb_to_hsv", "hsv_to_rgb"])
def test_restatement_hsv_equals_pillow_on_every_colour(direction):
    pytest.importorskip("PIL")
    pixels = _all_colours()
    fn, src, dst = (ac.rgb_to_hsv, "RGB", "HSV") if direction == "rgb_to_hsv" else (ac.hsv_to_rgb, "HSV", "RGB")
    want = _pil_convert(pixels, src, dst)
    step = 1 << 21  # chunks keep the float64 temporaries small
    for s in range(0, len(pixels), step):
        got = fn(pixels[s : s + step])
        assert np.array_equal(got, want[s : s + step]), (direction, s)


@pytest.mark.parametrize("op", ["brightness", "contrast", "saturation"])
def test_restatement_enhance_equals_pillow(op):
    Image = pytest.importorskip("PIL.Image")
    ImageEnhance = pytest.importorskip("PIL.ImageEnhance")
    enhancer = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}[op]
    frames = [ac.make_inputs(ac.BY_NAME["contrast_first"])[0][0], ac.flat_frame(113, 171, 3)]
    for frame in frames:
        for f in (0.6, 0.85, 1.0, 1.17, 1.4):
            want = np.asarray(enhancer(Image.fromarray(frame)).enhance(f))
            assert np.array_equal(getattr(ac, op)(frame, f), want), (op, f)


def test_restatement_hue_equals_pillow_round_trip():
    """torchvision's PIL adjust_hue, spelled with Pillow: split HSV, add uint8(f * 255) to H with wrap, merge, convert."""
    Image = pytest.importorskip("PIL.Image")
    frame = ac.flat_frame(113, 171, 3)
    frame[40:80, :160] = ac.make_inputs(ac.BY_NAME["contrast_first"])[0][0][40:80]
    for f in (-0.5 / 3.14, -0.07, 0.0, 0.1, 0.5 / 3.14):
        h, s, v = Image.fromarray(frame).convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over="ignore"):
            np_h = (np_h.astype(np.int32) + int(f * 255)).astype(np.uint8)  # wrap-around, as uint8 addition
        want = np.asarray(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
        assert np.array_equal(ac.hue(frame, f), want), f


# ------------------------------------------------------------------------------------------- the case table itself
def test_case_table_covers_what_it_claims():
    names = set(NAMES)
    assert {"contrast_first", "contrast_second", "contrast_third", "contrast_last"} <= names
    for pos, name in enumerate(["contrast_first", "contrast_second", "contrast_third", "contrast_last"]):
        assert ac.BY_NAME[name].params[0].order1.index(1) == pos
    # the stacked mean differs from the per-frame one: same inputs, same factors, different frames
    sym, asym = ac.expected("symmetric")[1], ac.expected("asymmetric")[1]
    assert not np.array_equal(sym[0], asym[0]) and not np.array_equal(sym[1], asym[1])
    assert np.array_equal(sym[2], asym[2])
    # flat regions put max == min pixels in front of the hue op
    flat = ac.make_inputs(ac.BY_NAME["contrast_third"])[0][0]
    assert (flat.max(-1) == flat.min(-1)).mean() > 0.2
    # the eraser changes the crop where it should and only there
    base = dataclasses.replace(ac.BY_NAME["rect_off_crop"].params[0], rects=())
    case = ac.BY_NAME["rect_off_crop"]
    i1, i2, fl, _ = ac.make_inputs(case)
    plain = ac.augment_sample(False, case.crop, i1[0], i2[0], fl[0], None, base)
    assert np.array_equal(plain[1], ac.expected("rect_off_crop")[1][1][0])
    one = ac.BY_NAME["one_rect"]
    i1, i2, fl, _ = ac.make_inputs(one)
    plain = ac.augment_sample(False, one.crop, i1[0], i2[0], fl[0], None, dataclasses.replace(one.params[0], rects=()))
    got = ac.expected("one_rect")[1]
    assert np.array_equal(plain[0], got[0][0]) and not np.array_equal(plain[1], got[1][0])
    # dense valid has zeros and ones where the flow holds values >= 1000
    v = ac.expected("big_flow")[1][3]
    assert 0 < v.sum() < v.size and (v[0] == 0).any() and (v[1] == 0).any()
    # sparse at 0.87: output pixels reached by more than one valid source
    reach = ac.expected("sparse_087")[2][0]
    shared = int((reach > 1).sum())
    print("sparse_087: pixels reached by more than one source:", shared)
    assert shared >= 20
    p = ac.BY_NAME["sparse_087"].params[0]
    win = reach[p.y0 : p.y0 + 64, p.x0 : p.x0 + 96]
    assert (win > 1).sum() >= 20  # ... and inside the crop
    # the clamps of the linear mapping are hit: first / last output index of an upscaled axis
    for name in ("scale_up_origin", "scale_up_last_row_col", "scale_odd_size"):
        c = ac.BY_NAME[name]
        q = c.params[0]
        ht1, wd1 = resized_size(*c.size, q)
        assert (q.y0 == 0 and q.x0 == 0) or (q.y0 + c.crop[0] == ht1 and q.x0 + c.crop[1] == wd1)
    q = ac.BY_NAME["scale_up_last_row_col"].params[0]
    assert np.float32((217 + 0.5) / q.scale_x - 0.5) >= 159 and np.float32((147 + 0.5) / q.scale_y - 0.5) >= 119


# ------------------------------------------------------------------------------------------- CPU path vs restatement
@pytest.mark.parametrize("name", NAMES)
def test_cpu_path_equals_restatement(name):
    case = ac.BY_NAME[name]
    got, want = _run(case)
    b, (ch, cw) = len(case.params), case.crop
    for k, (g, w, shape) in enumerate(zip(got, want, ((b, 3, ch, cw), (b, 3, ch, cw), (b, 2, ch, cw), (b, ch, cw)))):
        assert g.dtype == torch.float32 and tuple(g.shape) == shape and g.is_contiguous(), (name, k)
        assert np.array_equal(g.numpy(), w), (name, k, int((g.numpy() != w).sum()))


def test_to_tensor_packs_one_row_per_sample():
    rows = AugmentParams.to_tensor(ac.BY_NAME["batch3"].params)
    assert rows.dtype == torch.float64 and tuple(rows.shape) == (3, PARAM_DOUBLES) and rows.device.type == "cpu"
    r = rows[1].tolist()
    assert r[0] == 1.0 and r[1:5] == [3, 0, 1, 2] and r[9:13] == [0, 2, 1, 3] and r[17] == 2
    assert r[18:26] == [30, 20, 60, 55, 130, 90, 80, 70] and r[26] == 0 and r[30] == 1 and r[31:33] == [56, 64]
    assert rows[0, 27].item() == 0.75 and rows[0, 9:17].tolist() == rows[0, 1:9].tolist()  # symmetric: frame 2 = frame 1
    assert rows[:, 33:].abs().sum() == 0


# ------------------------------------------------------------------------------------------- sample()
def _seed(s):
    np.random.seed(s)
    torch.manual_seed(s)


@pytest.mark.parametrize("cls", [FlowAugmentor, SparseFlowAugmentor])
def test_sample_is_reproducible(cls):
    aug = cls((64, 96), do_flip=True)
    for s in range(20):
        _seed(s)
        a = aug.sample(120, 160)
        _seed(s)
        assert aug.sample(120, 160) == a
    _seed(1)
    assert aug.sample(120, 160) != a


def _replay_draws(rs, aug, p, ht, wd):
    """Advance ``rs`` by the np.random draws the docstrings of sample() list, deciding only from the draws themselves."""
    if not aug.sparse:
        rs.rand()
    if rs.rand() < 0.5:
        n = rs.randint(1, 3)
        for _ in range(n):
            rs.randint(0, wd), rs.randint(0, ht), rs.randint(50, 100), rs.randint(50, 100)
    rs.uniform(aug.min_scale, aug.max_scale)
    if not aug.sparse and rs.rand() < 0.8:
        rs.uniform(-0.2, 0.2), rs.uniform(-0.2, 0.2)
    rs.rand()
    if aug.do_flip:
        rs.rand()
        if not aug.sparse:
            rs.rand()
    ht1, wd1 = resized_size(ht, wd, p)
    if aug.sparse:
        rs.randint(0, ht1 - aug.crop_size[0] + 20), rs.randint(-50, wd1 - aug.crop_size[1] + 50)
    else:
        rs.randint(0, ht1 - aug.crop_size[0]), rs.randint(0, wd1 - aug.crop_size[1])


@pytest.mark.parametrize("cls,flip", [(FlowAugmentor, True), (FlowAugmentor, False), (SparseFlowAugmentor, True),
                                      (SparseFlowAugmentor, False)])
def test_sample_over_1000_seeds(cls, flip):
    aug = cls((64, 96), do_flip=flip)
    ht, wd, (ch, cw) = 120, 160, (64, 96)
    b, c, s, h = (0.3, 0.3, 0.3, 0.3 / 3.14) if aug.sparse else (0.4, 0.4, 0.4, 0.5 / 3.14)
    min_scale = max((ch + 1) / ht, (cw + 1) / wd) if aug.sparse else max((ch + 8) / ht, (cw + 8) / wd)
    seen = {"asym": 0, "resize": 0, "hflip": 0, "vflip": 0, "rects": set()}
    for seed in range(1000):
        _seed(seed)
        p = aug.sample(ht, wd)
        after = np.random.rand()
        rs = np.random.RandomState(seed)
        _replay_draws(rs, aug, p, ht, wd)
        assert rs.rand() == after, f"seed {seed}: sample() did not consume the documented np.random draws"
        ht1, wd1 = resized_size(ht, wd, p)
        assert 0 <= p.y0 <= ht1 - ch and 0 <= p.x0 <= wd1 - cw, (seed, p)
        for order, fac in ((p.order1, p.factors1), (p.order2, p.factors2)):
            assert sorted(order) == [0, 1, 2, 3]
            assert 1 - b <= fac[0] <= 1 + b and 1 - c <= fac[1] <= 1 + c and 1 - s <= fac[2] <= 1 + s
            assert -h <= fac[3] <= h
        if not p.asymmetric:
            assert p.order2 == p.order1 and p.factors2 == p.factors1
        assert len(p.rects) <= 2
        for x0, y0, dx, dy in p.rects:
            assert 0 <= x0 < wd and 0 <= y0 < ht and 50 <= dx < 100 and 50 <= dy < 100
        assert p.scale_x >= min_scale and p.scale_y >= min_scale and isinstance(p.scale_x, float)
        assert p.scale_x <= 2 ** (aug.max_scale + (0 if aug.sparse else aug.max_stretch)) + 1e-12
        if aug.sparse:
            assert not p.vflip and not p.asymmetric and p.scale_x == p.scale_y
        if not flip:
            assert not p.hflip and not p.vflip
        aug._validate(p, ht, wd)  # what sample() draws, augment_batch accepts
        seen["asym"] += p.asymmetric
        seen["resize"] += p.do_resize
        seen["hflip"] += p.hflip
        seen["vflip"] += p.vflip
        seen["rects"].add(len(p.rects))
    assert seen["rects"] == {0, 1, 2} and 700 < seen["resize"] < 900
    assert (seen["asym"] == 0) if aug.sparse else (120 < seen["asym"] < 280)
    assert (400 < seen["hflip"] < 600) if flip else seen["hflip"] == 0
    assert (50 < seen["vflip"] < 160) if (flip and not aug.sparse) else seen["vflip"] == 0


def test_colour_draws_follow_the_documented_order():
    aug = FlowAugmentor((64, 96))
    for seed in range(50):
        _seed(seed)
        p = aug.sample(120, 160)
        torch.manual_seed(seed)
        for order, fac in ((p.order1, p.factors1), (p.order2, p.factors2))[: 2 if p.asymmetric else 1]:
            assert tuple(int(v) for v in torch.randperm(4)) == order
            for v, (lo, hi) in zip(fac, ((0.6, 1.4), (0.6, 1.4), (0.6, 1.4), (-0.5 / 3.14, 0.5 / 3.14))):
                assert float(torch.empty(1).uniform_(lo, hi)) == v


def test_constructor_attributes_match_the_reference():
    d, s = FlowAugmentor((368, 768)), SparseFlowAugmentor((288, 960))
    for a, flip in ((d, True), (s, False)):
        assert (a.min_scale, a.max_scale, a.do_flip) == (-0.2, 0.5, flip)
        assert (a.spatial_aug_prob, a.stretch_prob, a.max_stretch) == (0.8, 0.8, 0.2)
        assert (a.h_flip_prob, a.v_flip_prob, a.asymmetric_color_aug_prob, a.eraser_aug_prob) == (0.5, 0.1, 0.2, 0.5)
    assert d.crop_size == (368, 768) and FlowAugmentor((8, 8), 0.1, 0.2, False).do_flip is False


def test_call_returns_the_per_sample_arrays():
    rng = np.random.default_rng(0)
    img1, img2 = (rng.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(2))
    flow = rng.standard_normal((120, 160, 2)).astype(np.float32)
    valid = (rng.random((120, 160)) < 0.3).astype(np.float32)
    keep = img2.copy()
    for seed in range(6):
        _seed(seed)
        o1, o2, fl = FlowAugmentor((64, 96))(img1, img2, flow)
        assert o1.shape == o2.shape == (64, 96, 3) and o1.dtype == o2.dtype == np.uint8
        assert fl.shape == (64, 96, 2) and fl.dtype == np.float32
        assert all(a.flags.c_contiguous for a in (o1, o2, fl))
        _seed(seed)
        o1, o2, fl, va = SparseFlowAugmentor((64, 96), do_flip=True)(img1, img2, flow, valid)
        assert o1.shape == o2.shape == (64, 96, 3) and o1.dtype == np.uint8 and fl.shape == (64, 96, 2)
        assert va.shape == (64, 96) and set(np.unique(va)) <= {0.0, 1.0}
    assert np.array_equal(img2, keep)  # the caller's frame is not erased in place
    _seed(3)
    p = FlowAugmentor((64, 96)).sample(120, 160)
    _seed(3)
    o1, _, fl = FlowAugmentor((64, 96))(img1, img2, flow)
    want = ac.augment_sample(False, (64, 96), img1, img2, flow.transpose(2, 0, 1), None, p)
    assert np.array_equal(o1.transpose(2, 0, 1), want[0]) and np.array_equal(fl.transpose(2, 0, 1), want[2])


# ------------------------------------------------------------------------------------------- checks before a launch
def _batch(b=2, ht=120, wd=160, device="cpu"):
    return (torch.zeros(b, ht, wd, 3, dtype=torch.uint8, device=device), torch.zeros(b, ht, wd, 3, dtype=torch.uint8, device=device),
            torch.zeros(b, 2, ht, wd, device=device), torch.ones(b, ht, wd, device=device))


def test_augment_batch_rejects_malformed_parameters():
    aug, sp = FlowAugmentor((64, 96)), SparseFlowAugmentor((64, 96))
    i1, i2, fl, va = _batch()
    ok = ac.P(y0=0, x0=0)
    bad = [
        ac.P(y0=57, x0=0), ac.P(y0=0, x0=65), ac.P(y0=-1, x0=0),  # the crop leaves the frame
        ac.P(do_resize=True, scale_x=0.65, scale_y=0.65, y0=15, x0=0),  # ... the resized frame (78 x 104)
        ac.P(do_resize=True, scale_x=0.0, scale_y=1.0), ac.P(do_resize=True, scale_x=1.0, scale_y=-1.0),
        ac.P(do_resize=True, scale_x=float("nan"), scale_y=1.0),
        ac.P(order=(0, 1, 2, 2)), ac.P(order=(0, 1, 2, 4)), ac.P(order=(0, 1, 2)),
        ac.P(order=(0, 1, 2, 3), order2=(1, 1, 1, 1), asym=True),
        ac.P(rects=((0, 0, 50, 50),) * 3), ac.P(rects=((-1, 0, 50, 50),)), ac.P(rects=((0, 0, 50.5, 50),)),
        ac.P(fac=(1.0, float("inf"), 1.0, 0.0)),
    ]
    for p in bad:
        with pytest.raises(ValueError, match="augment_batch"):
            aug.augment_batch(i1, i2, fl, params=[ok, p])
    with pytest.raises(ValueError, match="never flips vertically"):
        sp.augment_batch(i1, i2, fl, va, params=[ok, ac.P(vflip=True)])
    with pytest.raises(ValueError, match="parameter sets"):
        aug.augment_batch(i1, i2, fl, params=[ok])
    with pytest.raises(TypeError):
        aug.augment_batch(i1, i2, fl, params=[ok, {"y0": 0}])


def test_augment_batch_rejects_malformed_inputs():
    aug, sp = FlowAugmentor((64, 96)), SparseFlowAugmentor((64, 96))
    i1, i2, fl, va = _batch()
    ps = [ac.P(), ac.P()]
    with pytest.raises(ValueError):
        aug.augment_batch(i1[:, :, :, :2], i2, fl, params=ps)
    with pytest.raises(ValueError):
        aug.augment_batch(i1, i2[:1], fl, params=ps)
    with pytest.raises(ValueError):
        aug.augment_batch(i1, i2, fl.permute(0, 2, 3, 1), params=ps)
    with pytest.raises(TypeError):
        aug.augment_batch(i1.float(), i2.float(), fl, params=ps)
    with pytest.raises(TypeError):
        aug.augment_batch(i1, i2, fl.double(), params=ps)
    with pytest.raises(TypeError):
        aug.augment_batch(i1.numpy(), i2, fl, params=ps)
    with pytest.raises(ValueError):
        aug.augment_batch(i1, i2, fl, va, params=ps)  # the dense class takes no valid
    with pytest.raises(TypeError):
        sp.augment_batch(i1, i2, fl, None, params=ps)
    with pytest.raises(ValueError):
        sp.augment_batch(i1, i2, fl, va[:, :-1], params=ps)
    with pytest.raises(ValueError):
        sp.augment_batch(i1, i2, fl.to("meta"), va, params=ps)  # two devices
    out = aug.augment_batch(i1, i2, fl)  # default: sample() per sample
    assert tuple(out[0].shape) == (2, 3, 64, 96) and tuple(out[3].shape) == (2, 64, 96)


def test_operator_meta_kernel_and_no_cpu_fallback():
    from optical_flow import _native, _ops

    _native.load()
    assert "augment_batch" in _ops.OPS
    m = lambda *s, dt=torch.float32: torch.empty(*s, device="meta", dtype=dt)  # noqa: E731
    op = torch.ops.oflow.augment_batch
    i1, i2, fl, va, pa = (m(3, 120, 160, 3, dt=torch.uint8), m(3, 120, 160, 3, dt=torch.uint8), m(3, 2, 120, 160),
                          m(3, 120, 160), m(3, PARAM_DOUBLES, dt=torch.float64))
    for valid in (None, va):
        outs = op(i1, i2, fl, valid, pa, 64, 96)
        assert [tuple(o.shape) for o in outs] == [(3, 3, 64, 96), (3, 3, 64, 96), (3, 2, 64, 96), (3, 64, 96)]
        assert all(o.dtype == torch.float32 and o.device.type == "meta" for o in outs)
    for args in ((i1.float(), i2, fl, None, pa, 64, 96), (i1, i2, fl[:, :1], None, pa, 64, 96),
                 (i1, i2, fl, None, pa[:, :-1], 64, 96), (i1, i2, fl, None, pa.float(), 64, 96),
                 (i1, i2, fl, va[:2], pa, 64, 96), (i1, i2, fl, None, pa, 0, 96), (i1, i2[:, :-1], fl, None, pa, 64, 96)):
        with pytest.raises(RuntimeError, match="augment_batch"):
            op(*args)
    c = _batch(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        op(c[0], c[1], c[2], None, torch.zeros(1, PARAM_DOUBLES, dtype=torch.float64), 64, 96)


def test_c_abi_argument_errors_without_launch():
    from optical_flow import _native

    lib = _native.load()
    for name in ("oflow_augment_stats_u8", "oflow_augment_dense_f32", "oflow_augment_sparse_flow_f32"):
        assert name in _native.SYMBOLS
    p = 4096  # never dereferenced: every call below fails its checks first
    assert lib.oflow_augment_stats_u8(None, p, p, 1, 8, 8, 0, p, None) == -1
    assert lib.oflow_augment_stats_u8(p, p, None, 1, 8, 8, 0, p, None) == -1
    assert lib.oflow_augment_stats_u8(p, p, p, 1, 8, 8, 0, None, None) == -1
    for b, h, w, stage in ((0, 8, 8, 0), (1, 0, 8, 0), (1, 8, -1, 0), (65536, 8, 8, 0), (1, 1 << 15, 1 << 14, 0), (1, 8, 8, 2)):
        assert lib.oflow_augment_stats_u8(p, p, p, b, h, w, stage, p, None) == -2, (b, h, w, stage)
    assert lib.oflow_augment_dense_f32(p, None, p, p, p, 1, 8, 8, 4, 4, p, p, p, p, None) == -1
    assert lib.oflow_augment_dense_f32(p, p, p, p, p, 1, 8, 8, 4, 4, p, p, None, p, None) == -1  # flow without its output
    assert lib.oflow_augment_dense_f32(p, p, p, p, None, 1, 8, 8, 4, 4, p, p, p, p, None) == -1
    for b, h, w, ch, cw in ((0, 8, 8, 4, 4), (1, 8, 8, 0, 4), (1, 8, 8, 4, -4), (1, 8, 0, 4, 4), (1, 8, 8, 1 << 15, 1 << 14)):
        assert lib.oflow_augment_dense_f32(p, p, p, p, p, b, h, w, ch, cw, p, p, p, p, None) == -2, (b, h, w, ch, cw)
        assert lib.oflow_augment_sparse_flow_f32(p, p, p, b, h, w, ch, cw, p, p, None) == -2, (b, h, w, ch, cw)
    assert lib.oflow_augment_sparse_flow_f32(p, None, p, 1, 8, 8, 4, 4, p, p, None) == -1
    assert lib.oflow_augment_sparse_flow_f32(p, p, p, 1, 8, 8, 4, 4, p, None, None) == -1
