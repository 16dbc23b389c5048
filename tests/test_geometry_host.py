"""What each geometry of tests/geometry_cases.py is there for, pinned on the reference alone (oracle/servo_ref.py; no GPU).

tests/test_gpu_geometry.py compares the device with the oracle at these geometries.  A comparison can only fail where the thing
that may be wrong makes a difference: half-away rounding only at a rounding tie, another order of the fp64 operations only where
the two orders round differently, a wrong bounds test only with a pixel on the image's edge, a padded row's depth only where
depth[0, 0] is no hole.  The counts below are those conditions.  They are properties of the reference's arithmetic, so a change
of a geometry or of a case's seed that loses one fails here, before a device test loses its edge silently."""
import numpy as np
import pytest

import geometry_cases as gc
import homography_ref as hr
import law_support as ls
import pose_ref as pr
import robust_ref as rr


def _axis(name, axis):
    geo = gc.geometry(name)
    p = gc.products(geo, axis)
    ref = gc.round_reference(p)
    return dict(p=p, ref=ref, ties=int(gc.exact_ties(p).sum()), near=int(gc.near_ties(p).sum()),
                half_away=int((gc.round_half_away(p) != ref).sum()),
                product_first=int((gc.round_reference(gc.products(geo, axis, "product_first")) != ref).sum()))


def test_the_map_restated_per_axis_is_the_oracles():
    """products + round_reference, per axis, give calculate_uv's pixels: the counts below are about the oracle's own map."""
    for name in gc.GEOMETRIES:
        geo = gc.geometry(name)
        uv = gc.token_pixels(geo)
        idx = np.arange(geo.tokens)
        assert np.array_equal(uv[:, 0], _axis(name, "u")["ref"][idx % geo.grid]), name
        assert np.array_equal(uv[:, 1], _axis(name, "v")["ref"][idx // geo.grid]), name


@pytest.mark.parametrize("name,grid,moved_u,moved_v", [("ties14", 14, 7, 7), ("ties17", 17, 9, 8)])
def test_every_token_is_a_rounding_tie(name, grid, moved_u, moved_v):
    """Every product is an exact tie on both axes, so all T tokens are; half-away rounding moves about half the columns and rows."""
    geo = gc.geometry(name)
    u, v = _axis(name, "u"), _axis(name, "v")
    assert geo.grid == grid and u["ties"] == v["ties"] == grid and u["near"] == v["near"] == 0
    assert (u["half_away"], v["half_away"]) == (moved_u, moved_v)
    assert u["product_first"] == v["product_first"] == 0            # (these sizes do not tell the two orders apart)
    assert (geo.tokens > 256) == (name == "ties17")                  # the prefetched and the direct depth path


def test_near308_tells_the_orders_of_the_fp64_operations_apart():
    u, v = _axis("near308", "u"), _axis("near308", "v")
    assert (u["ties"], u["near"], u["product_first"]) == (7, 15, 6)
    assert (v["ties"], v["near"], v["product_first"]) == (22, 0, 0)
    assert u["half_away"] > 0 and v["half_away"] == 11


@pytest.mark.parametrize("name,n_outside", [("tiny", 27), ("tiny17", 33)])
def test_tiny_has_pixels_outside_shared_pixels_and_the_origin(name, n_outside):
    geo = gc.geometry(name)
    uv = gc.token_pixels(geo)
    out = gc.outside(geo, uv)
    assert int(out.sum()) == n_outside
    assert np.all((uv[out, 0] == geo.u_max) | (uv[out, 1] == geo.v_max))          # exactly ON the edge: u == u_max or v == v_max
    last = np.arange(geo.tokens)
    assert out[last % geo.grid == geo.grid - 1].all() and out[last // geo.grid == geo.grid - 1].all()   # the last column and row
    assert len(set(_axis(name, "v")["ref"].tolist())) == 10 and len({tuple(p) for p in uv.tolist()}) == 140   # shared pixels
    assert (uv == 0).all(axis=1).any()                                              # pixel (0, 0) is a patch centre


def test_portrait_hd_and_the_control():
    p, hd, base = gc.geometry("portrait"), gc.geometry("hd"), gc.geometry("base")
    pu, pv = ls.pitches(p.params(), p.patch, p.img)
    assert pv > pu
    uv = gc.token_pixels(hd)
    assert int((uv[:, 1] * hd.u_max + uv[:, 0]).max()) > 16 * 2 ** 16
    for axis in "uv":
        a = _axis("base", axis)
        assert a["ties"] == a["near"] == a["half_away"] == a["product_first"] == 0
    uv = gc.token_pixels(base)
    assert not gc.outside(base, uv).any() and not (uv == 0).all(axis=1).any() and tuple(uv.max(axis=0)) == (617, 463)


@pytest.mark.parametrize("name", list(gc.GEOMETRIES))
def test_depth_images_keep_their_border(name):
    geo = gc.geometry(name)
    rng = np.random.default_rng(1)
    d = gc.depth_image(geo, rng)
    assert d.shape == (geo.v_max, geo.u_max) and d.dtype == np.uint16
    assert d[0, 0] != 0 and d[-1].all() and d[:, -1].all() and d[:, 0].all()
    assert geo.v_max < 12 or np.count_nonzero(d == 0) > d.size // 10                # and holes inside
    assert gc.depth_image(geo, rng, level=137)[0, 0] != d[0, 0]


@pytest.mark.parametrize("name", list(gc.GEOMETRIES))
def test_table_cases_reach_what_they_are_for(name):
    geo = gc.geometry(name)
    cases = {mode: gc.table_case(name, mode) for mode in gc.TABLE_MODES}
    for mode in ("order", "dense", "explicit", "padded"):
        c = cases[mode]
        assert ls.ldlt_passes(c["ref"]["L"]) and np.linalg.cond(c["ref"]["L"]) < 1e3 and c["ref"]["v_c"].any(), (name, mode)
    assert 2 * cases["dense"]["rows"] > 128                                           # L in the global workspace
    pad = cases["padded"]
    assert not pad["s_star"][gc.LIVE:].any() and not pad["s_uv"][gc.LIVE:].any()
    assert np.all(pad["ref"]["Z"][gc.LIVE:] == pad["depth"][0, 0] / 1000.0) and pad["depth"][0, 0] != 0   # a padded row reads a DEPTH
    few = cases["too_few"]
    assert not few["s_star"].any() and not few["s_uv"].any() and not few["ref"]["v_c"].any()
    if name.startswith("tiny"):
        for mode in ("order", "dense", "explicit", "padded"):
            c = cases[mode]
            out = gc.outside(geo, c["s_uv"][:len(c["ids"])])
            assert out.any() and np.all(c["ref"]["Z"][:len(c["ids"])][out] == 100.0), (name, mode)


@pytest.mark.parametrize("name", gc.BORDER_GEOMETRIES)
def test_border_cases_put_matches_on_the_edge(name):
    c = gc.border_case(name)
    geo, s = c["geo"], c["s_uv"]
    on_u, on_v = s[:, 0] == geo.u_max, s[:, 1] == geo.v_max
    assert on_u.sum() >= 6 and on_v.sum() >= 6 and (s[:, 0] == 0).sum() >= 6 and (s[:, 1] == 0).sum() >= 6
    assert np.all(c["ref"]["Z"][on_u | on_v] == 100.0)
    # one past the end of a row is the next row's first pixel, and that is a depth: a read there would not look like a hole
    rows = np.nonzero(on_u & (s[:, 1] < geo.v_max - 1))[0]
    assert len(rows) and c["depth"][s[rows, 1] + 1, 0].all()
    assert ls.ldlt_passes(c["ref"]["L"]) and np.linalg.cond(c["ref"]["L"]) < 1e3


@pytest.mark.parametrize("name", list(gc.ROBUST_CASES))
def test_robust_cases_depend_on_the_floor(name):
    """The floor sigma_min decides the twist in every case (the bar on the device is 1e-9); on "portrait" the pitch_v / f_y term is
    the larger one, so pitch_u alone gives another twist; with f_x = f_y exchanging the pitches cannot show, with f_x != f_y it does.
    No pair's t comes closer than 1e-6 to the rejection point (tests/test_gpu_robust_law.py's margin rule)."""
    c = gc.robust_case(name)
    geo, K = c["geo"], c["sc"]["K"]
    square = gc.ROBUST_CASES[name][2]
    assert (K[0] == K[1]) == square
    assert c["rob"]["margin"] >= 1e-6
    assert rr.rel_l2(c["no_floor"]["v_c"], c["rob"]["v_c"]) > 1e-6
    pu, pv = ls.pitches(c["params"], geo.patch, geo.img)
    if geo.name == "portrait":
        assert pv / K[1] > pu / K[0] or not square
    if name == "portrait":
        assert rr.rel_l2(c["u_only"]["v_c"], c["rob"]["v_c"]) > 1e-6
    if square:
        assert c["swapped"]["v_c"].tolist() == c["rob"]["v_c"].tolist()
    else:
        assert rr.rel_l2(c["swapped"]["v_c"], c["rob"]["v_c"]) > 1e-6 and c["swapped"]["margin"] >= 1e-6
    if geo.name == "tiny":
        assert gc.outside(geo, c["s_uv"]).any()


def test_the_homography_case_depends_on_the_pitches():
    """On the oracle's own feature rows: the homography law's floor is active on "portrait" and exchanging the pitches moves the
    twist far beyond the device test's 1e-9."""
    c = gc.law_case()
    geo, params, sc = c["geo"], c["params"], c["sc"]
    det = gc.oracle_details(c, 130)
    pitches = ls.pitches(params, geo.patch, geo.img)
    h = hr.homography_from_details(det, 0, 0, sc["K"], params.lambda_, 0.61, gc.LAW_ITERATIONS, *pitches)
    hs = hr.homography_from_details(det, 0, 0, sc["K"], params.lambda_, 0.61, gc.LAW_ITERATIONS, *gc.swapped_pitches(pitches))
    assert h["status"] == hr.OK and all(g >= 1e-4 for g in h["ratios"]) and all(g >= 1e-6 for g in h["gaps"]) and h["edge"] >= 1e-6
    assert np.abs(h["v"] - hs["v"]).max() > 1e-6


def test_the_pose_case_depends_on_the_pitches():
    """On the oracle's own feature rows: with the plane's own goal depth the pose law's floor is reached on "portrait" (without it
    the twist is another one), and exchanging the pitches moves the twist far beyond the device test's 1e-9; with the right and
    with the exchanged pitches every solve keeps its gap and no row comes within 1e-6 of the rejection point."""
    c = gc.pose_case()
    geo, params, sc = c["geo"], c["params"], c["sc"]
    det = gc.oracle_details(c, 130)
    pitches = ls.pitches(params, geo.patch, geo.img)
    table = ls.goal_table(c["goal_depth"], geo.grid, geo.img, params)
    assert table[sc["ids"]].all() and len(set(table[sc["ids"]].tolist())) > 1
    with np.errstate(all="ignore"):
        p, swapped, no_floor = (pr.pose_from_details(det, 0, 0, sc["K"], table, params.lambda_, gc.LAW_ITERATIONS, *pp)
                                for pp in (pitches, gc.swapped_pitches(pitches), (0.0, 0.0)))
    for law in (p, swapped):
        assert law["status"] == pr.OK and all(g >= 1e-6 for g in law["gaps"]) and law["edge"] >= 1e-6 and int(law["info"][0]) >= 12
    assert int(p["info"][2]) == gc.LAW_ITERATIONS
    assert np.abs(p["v"] - no_floor["v"]).max() > 1e-6
    assert np.abs(p["v"] - swapped["v"]).max() > 1e-6
