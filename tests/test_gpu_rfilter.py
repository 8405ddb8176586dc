"""The film's reconstruction filters on the device: k_splat / k_gather of borders 1, 2 and 3
against a numpy restatement of ImageBlock::put (tests/rfilter_ref.py, written from the
reference's lines), over crafted samples (hpt_film_splat_batch) and end to end.

The bound is the fp32 summation bound of a pixel's n terms, |gpu - want| <= n * 2^-24 *
sum |w * v| per pixel and channel (the weight channel has v = 1): nothing about it is measured,
and it holds where negative lobes cancel."""
import numpy as np
import pytest

import rfilter_ref
import scene_util
from mitsuba_amd import native, scenes

pytestmark = pytest.mark.gpu
f = np.float32
W, H = 70, 45           # 3 x 2 blocks, neither side a multiple of 32


@pytest.fixture(scope="module")
def ctx():
    """a prepared device context with a 70 x 45 film (the splat hook reads the frame from it)"""
    _, r, _ = scene_util.make("furball_marschner", 200, W, H, 5, device=0)
    yield r
    r.close()


def _samples(radius, n_spp, seed=1234):
    """(pos (H, W, n, 2), rgb (H, W, n, 3)) crafted per pixel p: sample 0 at p + 0, 1 at p + 0.5,
    2 at nextafter(p + 1, 0), 3 at the offsets that make pos - 0.5 -+ radius an integer, the rest
    random -- so every image corner and both sides of every block edge get every one of them"""
    rng = np.random.default_rng(seed)
    base = np.stack(np.broadcast_arrays(np.arange(W, dtype=f)[None, :, None], np.arange(H, dtype=f)[:, None, None]), -1)
    off = rng.random((H, W, n_spp, 2)).astype(f)
    off[:, :, 0] = 0.0
    off[:, :, 1] = 0.5
    off[:, :, 2] = 1.0
    off[:, :, 3, 0] = f((0.5 + float(radius)) % 1.0)   # pos.x - 0.5 - radius is an integer
    off[:, :, 3, 1] = f((0.5 - float(radius)) % 1.0)   # pos.y - 0.5 + radius is an integer
    pos = (base + off).astype(f)
    pos = np.minimum(pos, np.nextafter(base + f(1), f(0)))   # stays in its pixel
    assert (np.floor(pos) == base).all()
    # radiance: 0, 1e-3 .. 1e3, and a few invalid samples that must add nothing
    rgb = (10.0 ** rng.uniform(-3, 3, (H, W, n_spp, 3))).astype(f)
    rgb[rng.random((H, W, n_spp)) < 0.05] = 0.0
    bad = rng.random((H, W, n_spp))
    rgb[bad < 0.01, 0] = np.nan
    rgb[(bad >= 0.01) & (bad < 0.02), 1] = np.inf
    rgb[(bad >= 0.02) & (bad < 0.03), 2] = -0.25
    for y, x in ((0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (31, 31), (32, 32), (31, 64), (32, 63)):
        rgb[y, x, :3] = [[1.0, 2.0, 3.0]] * 3            # the corners and block edges keep valid samples
        rgb[y, x, 3, 1] = np.nan                         # ... next to an invalid one
    return pos, rgb


def _check(got, want, mag, cnt, what):
    bound = rfilter_ref.bound(mag, cnt)
    err = np.abs(got.astype(np.float64) - want)
    lit = bound > 0
    worst = (err[lit] / bound[lit]).max()
    print(what, "terms/pixel max", cnt.max(), "worst err / bound", worst, "pixels with cancellation",
          int((np.abs(want[..., 0]) < 0.5 * mag[..., 0]).sum()))
    assert np.isfinite(got).all()
    assert (err <= bound).all(), (what, worst, np.argwhere(err > bound)[:5])


_want = {}


def _case(ctx, kind, n_spp):
    """filter `kind` set on the context; its samples and numpy film, computed once"""
    ctx.set_rfilter(kind)
    if (kind, n_spp) not in _want:
        rf = ctx.rfilter()
        flt = (rf["lut"], rf["scale"], rf["radius"], rf["border"])
        pos, rgb = _samples(rf["radius"], n_spp)
        _want[kind, n_spp] = (pos, rgb) + rfilter_ref.put(pos, rgb, flt)
    return _want[kind, n_spp]


@pytest.mark.parametrize("kind,n_spp", [(k, 5) for k in rfilter_ref.KINDS] + [("gaussian", 260)])
def test_splat_against_imageblock_put(ctx, kind, n_spp):
    """260 samples: past the lane loop's 256 stride and no multiple of 64"""
    pos, rgb, want, mag, cnt = _case(ctx, kind, n_spp)
    assert cnt.min() >= 1
    if kind in ("mitchell", "catmullrom", "lanczos"):
        assert (want[..., 3] < mag[..., 3]).any()         # negative weights did reach pixels
    _check(ctx.film_splat(pos, rgb), want, mag, cnt, "%s x %d" % (kind, n_spp))


def test_box_sample_on_a_pixel_edge_reaches_both_pixels(ctx):
    """box.cpp:34-38: radius 0.5 + 1e-5, so a sample at x = 10 exactly lands in pixels 9 and 10"""
    ctx.set_rfilter("box")
    pos = np.zeros((H, W, 1, 2), f)
    pos[..., 0] = np.arange(W, dtype=f)[None, :, None] + f(0.5)
    pos[..., 1] = np.arange(H, dtype=f)[:, None, None] + f(0.5)
    rgb = np.full((H, W, 1, 3), -1.0, f)                  # every other sample is invalid
    pos[7, 10, 0] = (10.0, 7.5)
    rgb[7, 10, 0] = (1.0, 1.0, 1.0)
    film = ctx.film_splat(pos, rgb)
    ys, xs = np.nonzero(film[..., 3])
    assert sorted(zip(ys.tolist(), xs.tolist())) == [(7, 9), (7, 10)]
    rf = ctx.rfilter()
    want, mag, cnt = rfilter_ref.put(pos, rgb, (rf["lut"], rf["scale"], rf["radius"], rf["border"]))
    assert want[7, 9, 3] > 0 and want[7, 10, 3] > 0
    _check(film, want, mag, cnt, "box edge")


@pytest.mark.parametrize("kind", ["gaussian", "lanczos"])
def test_shards_and_waves_add_up_to_the_frame(ctx, kind):
    pos, rgb, want, mag, cnt = _case(ctx, kind, 5)
    one = ctx.film_splat(pos, rgb)
    shards = [ctx.film_splat(pos, rgb, shard=s, n_shards=3) for s in range(3)]
    own = [sh[..., 3] != 0 for sh in shards]
    assert all(o.any() for o in own) and (sum(o.astype(int) for o in own) > 1).any()   # footprints overlap
    total = np.sum([sh.astype(np.float64) for sh in shards], axis=0)
    _check(total, want, mag, cnt, kind + " 3 shards")
    bound = rfilter_ref.bound(mag, cnt)
    assert (np.abs(total - one.astype(np.float64)) <= bound).all()
    # 6 blocks x 1024 slots x 2 samples per wave: waves of 2, 2 and 1 samples per pixel
    waves = ctx.film_splat(pos, rgb, max_wave_paths=6 * 1024 * 2)
    _check(waves, want, mag, cnt, kind + " 3 waves")
    assert (np.abs(waves.astype(np.float64) - one) <= bound).all()
    # ... and in place: shard after shard accumulated into one film
    acc = np.zeros((H, W, 4), f)
    for s in range(3):
        ctx.film_splat(pos, rgb, shard=s, n_shards=3, max_wave_paths=2 * 1024 * 2, film=acc)
    _check(acc, want, mag, cnt, kind + " 3 shards x 3 waves, accumulated")


# ---- end to end ----

def _furball(rfilter="tent"):
    xml = scenes.make_scene("furball_marschner", scene_util.WORK, n_strands=1000, rfilter=rfilter)
    r = native.Renderer(device=0)
    r.load_scene_xml(xml, {"width": 64, "height": 64, "spp": 6, "maxDepth": scenes.CONFIGS["furball_marschner"]["max_depth"]})
    r.prepare()
    return r


@pytest.fixture(scope="module")
def frames():
    """the 64 x 64 x 6 furball with the tent (a context that never heard of hpt_set_rfilter), with
    the gaussian from the XML, and with the gaussian set on a prepared tent scene"""
    _, tent, _ = scene_util.make("furball_marschner", 1000, 64, 64, 6, device=0)
    out = {"tent": (tent.render(), tent.render_samples())}
    gx = _furball("gaussian")
    assert gx.scene_json()["sensor"]["rfilter"] == "gaussian"
    out["xml"] = (gx.render(), gx.render_samples())
    gs = _furball("tent")
    gs.set_rfilter("gaussian")
    out["set"] = (gs.render(), gs.render_samples())
    gs.set_rfilter(native.RFILTERS["tent"])
    out["back"] = (gs.render(), gs.render_samples())
    out["rfilter"] = gx.rfilter()
    for r in (tent, gx, gs):
        r.close()
    return out


def test_gaussian_from_xml_equals_gaussian_from_the_setter(frames):
    np.testing.assert_array_equal(frames["xml"][0], frames["set"][0])


def test_rendered_film_is_the_put_of_its_samples(frames):
    film, (pos, rgb) = frames["xml"]
    assert pos.shape == (64, 64, 6, 2) and (np.floor(pos[..., 0]) == np.arange(64)[None, :, None]).all()
    rf = frames["rfilter"]
    want, mag, cnt = rfilter_ref.put(pos, rgb, (rf["lut"], rf["scale"], rf["radius"], rf["border"]))
    assert (rgb.max(axis=-1) > 0).mean() > 0.25           # the furball covers a third of the frame
    _check(film, want, mag, cnt, "furball gaussian")


def test_filter_changes_the_film_and_nothing_upstream(frames):
    for a, b in zip(frames["xml"][1], frames["tent"][1]):
        np.testing.assert_array_equal(a, b)               # positions and radiance, bit for bit
    g, t = native.develop(frames["xml"][0]), native.develop(frames["tent"][0])
    assert np.abs(g - t).max() > 1e-3 and not np.array_equal(frames["xml"][0], frames["tent"][0])


def test_tent_film_is_unchanged_by_the_setter(frames):
    """hpt_set_rfilter(TENT), after a gaussian frame on the same context, gives the film of a
    context that never called it"""
    np.testing.assert_array_equal(frames["back"][0], frames["tent"][0])


def test_render_samples_need_a_single_wave():
    r = _furball()
    with pytest.raises(native.HairPTError) as e:
        r.render_samples()                                # nothing rendered yet
    assert e.value.code == -4
    r.render(max_wave_paths=4 * 1024 * 2)                 # 4 blocks, 2 of 6 samples per wave
    assert r.stats().waves == 3
    with pytest.raises(native.HairPTError) as e:
        r.render_samples()
    assert e.value.code == -4
    r.close()
