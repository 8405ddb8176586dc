"""The film's reconstruction filters on the host (no GPU): the LUT that hpt_set_rfilter /
<rfilter> configure against a float32 numpy restatement of the reference (tests/rfilter_ref.py),
the XML parser's handling of every plugin and parameter, and the defaults -- gaussian for a
<film> without <rfilter> (film.cpp:90-94), tent for a scene described through the setters."""
import os

import numpy as np
import pytest

import rfilter_ref
import scene_util
from mitsuba_amd import native, scenes

# (plugin, parameters as rfilter_ref.configure takes them, (p0, p1) of hpt_set_rfilter)
DEFAULTS = [(k, {}, (-1.0, -1.0)) for k in rfilter_ref.KINDS]
VARIANTS = [("gaussian", {"stddev": 0.75}, (0.75, -1.0)), ("lanczos", {"lobes": 2}, (2.0, -1.0)),
            ("mitchell", {"B": 0.0, "C": 1.0}, (0.0, 1.0)), ("box", {"radius": 1.0}, (1.0, -1.0))]
EXACT = ("box", "tent", "catmullrom")   # plain fp32 arithmetic: no libm call, no contraction


@pytest.fixture(scope="module")
def host():
    r = native.Renderer(device=native.HOST_ONLY)
    yield r
    r.close()


def test_host_code_is_built_without_contraction_or_fast_math():
    """the bit-equal cases below rest on it"""
    mk = open(os.path.join(native.PKG, "Makefile")).read()
    flags = [ln for ln in mk.splitlines() if ln.startswith("HOSTFLAGS")][0]
    assert "-ffp-contract=off" in flags and "-fno-fast-math" in flags and "-Ofast" not in flags


@pytest.mark.parametrize("kind,params,p", DEFAULTS + VARIANTS, ids=lambda v: v if isinstance(v, str) else None)
def test_lut_matches_the_reference_configure(host, kind, params, p):
    want_lut, want_scale, want_radius, want_border = rfilter_ref.configure(kind, **params)
    host.set_rfilter(kind, *p)
    got = host.rfilter()
    assert got["type"] == kind
    assert got["radius"] == want_radius and got["scale"] == want_scale and got["border"] == want_border
    assert got["lut"][31] == 0 and want_lut[31] == 0
    lut = got["lut"]
    if kind in EXACT:
        np.testing.assert_array_equal(lut, want_lut)
        return
    # 4 ulp of the entry (libm's expf / sinf, the cubic's cancellation), + 1e-7 for the entries
    # next to a zero crossing (a sign change, or a neighbour that is exactly zero)
    s = np.sign(want_lut)
    near_zero = np.zeros(32, bool)
    near_zero[1:] |= s[1:] != s[:-1]
    near_zero[:-1] |= s[:-1] != s[1:]
    tol = 4 * np.spacing(np.abs(want_lut)).astype(np.float64) + 1e-7 * near_zero
    err = np.abs(lut.astype(np.float64) - want_lut.astype(np.float64))
    print(kind, params, "max err / tol", (err / tol).max(), "bit-equal entries", int((lut == want_lut).sum()))
    assert (err <= tol).all(), (err / tol).max()
    if kind in ("mitchell", "lanczos"):
        assert lut.min() < 0  # negative lobes reach the film


def _scene(tmp_path, rfilter_xml):
    """a generated scene whose <rfilter .../> element is rfilter_xml ('' = none)"""
    xml = scenes.make_scene("furball_marschner", str(tmp_path), n_strands=50)
    text = open(xml).read()
    assert text.count('<rfilter type="tent"/>') == 1
    path = tmp_path / "rf.xml"
    path.write_text(text.replace('<rfilter type="tent"/>', rfilter_xml))
    return str(path)


PARSED = [
    ('<rfilter type="box"/>', {"rfilter": "box", "rfilterBoxRadius": 0.5, "rfilterRadius": 0.50001, "rfilterBorder": 1}),
    ('<rfilter type="box"><float name="radius" value="1.0"/></rfilter>',
     {"rfilter": "box", "rfilterBoxRadius": 1.0, "rfilterRadius": 1.00001, "rfilterBorder": 1}),
    ('<rfilter type="tent"/>', {"rfilter": "tent", "rfilterRadius": 1.0, "rfilterBorder": 1}),
    ('<rfilter type="gaussian"/>', {"rfilter": "gaussian", "rfilterStddev": 0.5, "rfilterRadius": 2.0, "rfilterBorder": 2}),
    ('<rfilter type="gaussian"><float name="stddev" value="0.75"/><float name="unknown" value="7"/></rfilter>',
     {"rfilter": "gaussian", "rfilterStddev": 0.75, "rfilterRadius": 3.0, "rfilterBorder": 3}),
    ('<rfilter type="mitchell"/>', {"rfilter": "mitchell", "rfilterB": 1 / 3, "rfilterC": 1 / 3, "rfilterRadius": 2.0,
                                    "rfilterBorder": 2}),
    ('<rfilter type="mitchell"><float name="B" value="0"/><float name="C" value="1"/></rfilter>',
     {"rfilter": "mitchell", "rfilterB": 0.0, "rfilterC": 1.0, "rfilterRadius": 2.0}),
    ('<rfilter type="catmullrom"/>', {"rfilter": "catmullrom", "rfilterRadius": 2.0, "rfilterBorder": 2}),
    ('<rfilter type="lanczos"/>', {"rfilter": "lanczos", "rfilterLobes": 3, "rfilterRadius": 3.0, "rfilterBorder": 3}),
    ('<rfilter type="lanczos"><integer name="lobes" value="2"/></rfilter>',
     {"rfilter": "lanczos", "rfilterLobes": 2, "rfilterRadius": 2.0, "rfilterBorder": 2}),
    ('', {"rfilter": "gaussian", "rfilterStddev": 0.5, "rfilterRadius": 2.0}),    # film.cpp:90-94
]


@pytest.mark.parametrize("rf,want", PARSED, ids=[w["rfilter"] + str(i) for i, (_, w) in enumerate(PARSED)])
def test_parser_round_trips_every_filter_into_the_json(host, tmp_path, rf, want):
    host.load_scene_xml(_scene(tmp_path, rf))
    sen = host.scene_json()["sensor"]
    for k, v in want.items():
        assert sen[k] == (pytest.approx(v, rel=1e-6) if isinstance(v, float) else v), (k, sen[k])
    got = host.rfilter()   # the loaded scene's filter is the context's
    assert got["type"] == want["rfilter"] and got["radius"] == pytest.approx(want["rfilterRadius"], rel=1e-6)


def test_defined_filter_type_is_substituted(host, tmp_path):
    xml = scenes.make_scene("furball_marschner", str(tmp_path), n_strands=50, rfilter="$rf")
    assert '<rfilter type="$rf"/>' in open(xml).read()
    host.load_scene_xml(xml, {"rf": "lanczos"})
    assert host.scene_json()["sensor"]["rfilter"] == "lanczos" and host.rfilter()["border"] == 3
    host.load_scene_xml(xml, {"rf": "catmullrom"})
    assert host.scene_json()["sensor"]["rfilter"] == "catmullrom"


def test_default_scene_xml_is_unchanged_by_the_keyword(tmp_path):
    a = open(scenes.make_scene("furball_marschner", str(tmp_path), n_strands=50)).read()
    b = open(scenes.make_scene("furball_marschner", str(tmp_path), n_strands=50, rfilter="tent")).read()
    assert a == b and '      <rfilter type="tent"/>\n' in a


REFUSED = [('<rfilter type="gaussian"><float name="stddev" value="1.0"/></rfilter>', "gaussian"),   # border 4
           ('<rfilter type="lanczos"><integer name="lobes" value="4"/></rfilter>', "lanczos"),
           ('<rfilter type="box"><float name="radius" value="0"/></rfilter>', "box"),
           ('<rfilter type="sinc"/>', "sinc")]


@pytest.mark.parametrize("rf,name", REFUSED, ids=[n for _, n in REFUSED])
def test_parser_refuses_what_the_device_film_cannot_hold(tmp_path, rf, name):
    r = native.Renderer(device=native.HOST_ONLY)
    with pytest.raises(native.HairPTError) as e:
        r.load_scene_xml(_scene(tmp_path, rf))
    assert e.value.code in (-1, -2) and name in str(e.value), str(e.value)


def test_setter_refuses_with_the_filter_radius_and_limit(host):
    with pytest.raises(native.HairPTError) as e:
        host.set_rfilter("gaussian", 1.0)
    assert e.value.code == -1
    msg = str(e.value)
    assert "gaussian" in msg and "radius 4" in msg and "limit of 3" in msg, msg
    for kind, p0 in (("lanczos", 4.0), ("lanczos", 0.0), ("box", 0.0), ("gaussian", 0.0)):
        with pytest.raises(native.HairPTError) as e:
            host.set_rfilter(kind, p0)
        assert e.value.code == -1 and kind in str(e.value)
    with pytest.raises(native.HairPTError):
        host.set_rfilter(6)


def test_setter_path_defaults_to_the_tent():
    r = native.Renderer(device=native.HOST_ONLY)
    got = r.rfilter()
    assert (got["type"], got["radius"], got["border"]) == ("tent", 1.0, 1)
    np.testing.assert_array_equal(got["lut"], rfilter_ref.configure("tent")[0])
    r.set_sampler(4)                         # other setters leave it alone
    assert r.rfilter()["type"] == "tent"


def test_setter_works_after_prepare_without_another_prepare():
    _, r, _ = scene_util.make("furball_marschner", 50, 16, 16, 1)
    assert r.rfilter()["type"] == "tent"     # (that scene's XML spells the tent out)
    nodes = r.info().kd_nodes
    r.set_rfilter("mitchell", 0.0, 1.0)
    assert r.rfilter()["type"] == "mitchell" and r.info().kd_nodes == nodes > 0
