"""Hand cases for tests/ref_stereo.py, the checker of plba_stereo_associate, with the expected values worked
out here; the condition on the generated cases (every gate and the window's asymmetry reject and pass rows,
a quarter of the largest case survives); and plslam_stereo_cpu against the checker, bit for bit. No GPU."""
import numpy as np
import pytest

import ref_stereo as RS
import stereo_cases as SC
from plba import capi, slam_map

# a camera with exactly representable values, so that the expected doubles below are exact by hand
CAM = SC.HAND_CAMERA


def prm(**kw):
    return RS.params(**CAM, **kw)


desc = SC.bits_desc


def pts(left, right, dl=None, dr=None):
    return dict(pt_l=np.array(left, np.float32).reshape(-1, 2), pt_r=np.array(right, np.float32).reshape(-1, 2),
                pdesc_l=np.array(dl if dl is not None else [desc()] * len(left)),
                pdesc_r=np.array(dr if dr is not None else [desc()] * len(right)))


def lns(left, right):
    return dict(ls_l=np.array(left, np.float32).reshape(-1, 4), ls_r=np.array(right, np.float32).reshape(-1, 4),
                ldesc_l=np.array([desc()] * len(left)), ldesc_r=np.array([desc()] * len(right)))


def test_point_pair_that_passes():
    r = RS.associate(pts([(328.0, 248.0)], [(320.0, 248.5)]), prm())
    assert r["n_pt"] == 1 and r["pt_src"].tolist() == [0]
    # disp = 8, bd = 0.125 / 8 = 1 / 64; P = (8 / 64, 8 / 64, 512 / 64)
    assert r["pt_pl"].tolist() == [[328.0, 248.0]] and r["pt_disp"].tolist() == [8.0]
    assert r["pt_P"].tolist() == [[0.125, 0.125, 8.0]]
    assert r["pdesc"].tobytes() == desc().tobytes()


@pytest.mark.parametrize("right, gate", [((320.0, 249.5), "epipolar"), ((327.5, 248.0), "disparity")])
def test_point_rejected_by_one_gate_alone(right, gate):
    # |dy| = 1.5 > 1 with disp 8 >= 1; disp 0.5 < 1 with dy 0
    bits = RS.point_row(prm(), np.float32([328.0, 248.0]), np.float32(right))[0]
    assert bits == {"epipolar": 1, "disparity": 2}[gate]
    assert RS.associate(pts([(328.0, 248.0)], [right]), prm())["n_pt"] == 0
    # at the bounds themselves the reference accepts: <= max_dist_epip, >= min_disp
    assert RS.point_row(prm(), np.float32([328.0, 248.0]), np.float32([327.0, 249.0]))[0] == 0


def test_window_is_asymmetric():
    """The query cell of (328, 248) is (32, 24): 10 px a cell. A right point one cell to the right (cell 33)
    and one a row below (row 25) are nearer in Hamming distance than the true partner in cell 31, and a
    symmetric window would take them; the stereo window [x - 10, x] x [y, y] must not."""
    left, dl = [(328.0, 248.0)], [desc(0, 1, 2, 3)]
    frames = SC.asymmetric_window_frames()
    for f in frames:
        r = RS.associate(f, prm())
        assert r["n_pt"] == 1 and r["pt_disp"].tolist() == [10.0]              # matched to the true partner
        stats = {}
        RS.associate(f, prm(), stats)
        assert stats["window_reject"] == 1 and stats["window_pass"] == 1
        # the same frame with a symmetric window of one cell would take the decoy: disparity -10 or 0, rejected
        assert RS.point_row(prm(), f["pt_l"][0], f["pt_r"][0])[0] & 2
    # the CPU restatement, single calls and one batch
    for got in [slam_map.stereo_cpu([f], prm())[0] for f in frames] + slam_map.stereo_cpu(frames, prm()):
        assert got["n_pt"] == 1 and got["pt_disp"].tolist() == [10.0] and got["pt_src"].tolist() == [0]
    # the window reaches matching_s_ws cells to the left and not one further
    far = pts(left, [(328.0 - 105.0, 248.0)], dl, [desc(0, 1, 2, 3)])           # cell 22 = 32 - 10
    assert RS.associate(far, prm(matching_s_ws=10))["n_pt"] == 1
    assert RS.associate(far, prm(matching_s_ws=9))["n_pt"] == 0


# the left segment (330, 100) -> (300, 200) and a right one 10 px to the left of it, a little longer
LEFT = (330.0, 100.0, 300.0, 200.0)
RIGHT = (323.0, 90.0, 287.0, 210.0)   # x = 350 - 0.3 y at y = 90 and y = 210


def test_line_survivor_by_hand():
    r = RS.associate(lns([LEFT], [RIGHT]), prm(pluker=1))
    assert r["n_ls"] == 1 and r["ls_src"].tolist() == [0]
    # :367  X  = (323 * (100 - 210) + 287 * (90 - 100)) / (90 - 210) = (-35530 - 2870) / -120 = 320
    # :368  Xe = (320 * (200 - 210) + 287 * (100 - 200)) / (100 - 210) = (-3200 - 28700) / -110 = 290
    assert r["ls_sdisp"].tolist() == [10.0] and r["ls_edisp"].tolist() == [10.0]
    assert r["ls_spl"].tolist() == [[330.0, 100.0]] and r["ls_epl"].tolist() == [[300.0, 200.0]]
    bd = 0.125 / 10.0
    assert r["ls_sP"].tolist() == [[bd * 10.0, bd * -140.0, bd * 512.0]]
    assert r["ls_eP"].tolist() == [[bd * -20.0, bd * -40.0, bd * 512.0]]
    # le = (100 - 200, 300 - 330, 330 * 200 - 100 * 300) / sqrt(100^2 + 30^2)
    n = np.sqrt(np.float64(10900.0))
    assert r["ls_le"].tolist() == [[-100.0 / n, -30.0 / n, 36000.0 / n]]
    # the two viewing planes. a = ((330 - 320) / 512, (100 - 240) / 256, 1), c = (-20 / 512, -40 / 256, 1);
    # pi1 = (a x c, -0); a2 = (0 / 512 + b, a_y, 1), c2 = (-30 / 512 + b, c_y, 1); pi2 = ((a2 - o2) x (c2 - o2), -(b * (a2 x c2)_x))
    a, c = np.array([10 / 512, -140 / 256, 1.0]), np.array([-20 / 512, -40 / 256, 1.0])
    a2, c2 = np.array([0 / 512 + 0.125, -140 / 256, 1.0]), np.array([-30 / 512 + 0.125, -40 / 256, 1.0])
    o2 = np.array([0.125, 0.0, 0.0])

    def cross(u, v):
        return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]])
    pi1 = np.append(cross(a, c), -0.0)
    x = cross(a2, c2)
    pi2 = np.append(cross(a2 - o2, c2 - o2), -(0.125 * x[0] + (0.0 * x[1] + 0.0 * x[2])))
    dp = np.outer(pi1, pi2) - np.outer(pi2, pi1)
    assert r["ls_NDc"].tolist() == [[dp[0, 3], dp[1, 3], dp[2, 3], -dp[1, 2], dp[0, 2], -dp[0, 1]]]
    # the line is the intersection of the planes: its direction is orthogonal to both normals
    d = r["ls_NDc"][0, 3:]
    assert abs(d @ pi1[:3]) < 1e-12 and abs(d @ pi2[:3]) < 1e-12
    assert "ls_NDc" not in RS.associate(lns([LEFT], [RIGHT]), prm(pluker=0))


def shifted(ds, de, u0=0.0, u1=1.0):
    """A right segment on the line that lies ds (de) to the left of LEFT at its start (end), from the height
    u0 to the height u1 of the left segment."""
    sx, sy, ex, ey = LEFT

    def at(u):
        return sx + u * (ex - sx) - (ds + u * (de - ds)), sy + u * (ey - sy)
    return at(u0) + at(u1)


@pytest.mark.parametrize("left, right, bits", [
    (LEFT, shifted(0.75, 1.0), 1),                    # sdisp = 0.75 < 1 alone; the ratio 0.75 >= 0.7 resets nothing
    (LEFT, shifted(1.25, 0.9375), 2),                 # edisp < 1 alone, ratio 0.75
    ((330.0, 100.0, 300.0, 100.0625), (320.0, 100.0, 290.0, 100.0625), 4 | 8),   # a horizontal left line: the third and the
                                                                             # fourth gate, which can only fall together
    (LEFT, shifted(10.0, 10.0, 0.0, 0.5), 16),        # the right segment covers half of the left: overlap 0.5
])
def test_line_rejected_by_one_gate_alone(left, right, bits):
    got = RS.line_row(prm(), np.float32(left), np.float32(right))[0]
    assert got == bits
    assert RS.associate(lns([left], [right]), prm())["n_ls"] == 0


def test_fourth_gate_sees_the_left_line():
    """After :367-368 sp_r(1) = sy_l and ep_r(1) = ey_l, so the fourth gate repeats the third: a right
    segment that is itself horizontal (sy_r - ey_r = 0.05) does not trip it when the left one is not ..."""
    right = (321.0, 149.975, 319.0, 150.025)
    bits, o = RS.line_row(prm(), np.float32(LEFT), np.float32(right))
    assert bits & (4 | 8) == 0
    # ... and over the generated cases both bits are always equal
    stats = {}
    for name in SC.CASES:
        RS.associate(SC.case(name), RS.params(**SC.CAMERA), stats)
    assert stats["horiz_l_reject"] == stats["horiz_r_reject"] > 0


def test_ep_r_reads_the_overwritten_sp_r():
    """:368 reads the sp_r that :367 wrote, (X, sy_l), not the right segment's own start. Both readings put
    ep_r on the same right line at the height ey_l, so in exact arithmetic they agree; in double they round
    differently, and the output must carry the reference's rounding. (What the overwrite changes beyond the
    last bit is the fourth gate, test_fourth_gate_sees_the_left_line.)"""
    l, r = np.float32(LEFT), np.float32((317.2, 86.2, 291.0, 211.5))
    slx, sly, elx, ely = (np.float64(v) for v in l)
    srx, sry, erx, ery = (np.float64(v) for v in r)
    X = (srx * (sly - ery) + erx * (sry - sly)) / (sry - ery)
    new = (X * (ely - ery) + erx * (sly - ely)) / (sly - ery)
    old = (srx * (ely - ery) + erx * (sry - ely)) / (sry - ery)
    assert new != old and abs(new - old) < 1e-12
    p = prm(ls_min_disp_ratio=0.0)   # the two disparities differ by more than the default ratio allows
    bits, o = RS.line_row(p, l, r)
    assert bits == 0 and o["sdisp"] == slx - X and o["edisp"] == elx - new and o["edisp"] != elx - old
    got = slam_map.stereo_cpu([lns([l], [r])], p)[0]
    assert got["n_ls"] == 1 and got["ls_edisp"][0] == elx - new


def test_nan_in_a_gate_compares_false():
    # a right segment with sy_r == ey_r: X = x / 0; every comparison with the NaN or the infinity is decided as C++ does
    bits, _ = RS.line_row(prm(), np.float32(LEFT), np.float32((320.0, 150.0, 290.0, 150.0)))
    assert bits & 3


@pytest.fixture(scope="module")
def generated():
    """name -> (frame, checker's result) for the default flags, computed once, with the gate statistics."""
    stats, out = {}, {}
    for name in SC.CASES:
        f = SC.case(name)
        out[name] = (f, RS.associate(f, RS.params(**SC.CAMERA, pluker=1), stats))
    return out, stats


def test_generator_exercises_every_gate(generated):
    out, stats = generated
    for g in RS.PT_GATES + RS.LS_GATES + ("window",):
        assert stats[g + "_reject"] > 0 and stats[g + "_pass"] > 0, (g, stats)
    f, r = out[SC.LARGEST]
    assert max(len(f.get("pt_l", ())) for f, _ in out.values()) == len(f["pt_l"])
    assert 4 * r["n_pt"] >= len(f["pt_l"]), r["n_pt"]
    assert out["lines_40x40"][1]["n_ls"] > 0 and out["lines_outside"][1]["n_ls"] > 0


@pytest.mark.parametrize("pluker", [0, 1])
@pytest.mark.parametrize("best_lr", [0, 1])
def test_stereo_cpu_equals_checker(generated, best_lr, pluker):
    p = RS.params(**SC.CAMERA, best_lr=best_lr, pluker=pluker)
    frames = [SC.case(n) for n in SC.CASES]
    got = slam_map.stereo_cpu(frames, p)                      # one batch of all the cases
    for name, f, g in zip(SC.CASES, frames, got):
        w = generated[0][name][1] if (best_lr, pluker) == (1, 1) else RS.associate(f, p)
        assert RS.same(w, g) is None, name
        assert RS.same(slam_map.stereo_cpu([f], p)[0], g) is None, name


def test_c_defaults_are_those_of_the_checker():
    """plba_stereo_default_params, which every Python call starts from, against the checker's own table
    (src2/config.cpp:51-91); what has no default is zero."""
    p = capi.stereo_params()
    got = {k: getattr(p, k) for k, _ in capi.PlbaStereoParams._fields_}
    assert got == dict(RS.DEFAULTS, width=0, height=0, pad=0, fx=0.0, fy=0.0, cx=0.0, cy=0.0, b=0.0)
    q = capi.stereo_params(dict(width=7, min_disp=2.5))
    assert (q.width, q.min_disp, q.matching_s_ws) == (7, 2.5, 10)
    with pytest.raises(KeyError):
        capi.stereo_params(dict(no_such_field=1))


def test_stereo_cpu_refusals():
    f = SC.case("mixed")
    p = RS.params(**SC.CAMERA)
    for key, v in (("pt_l", np.nan), ("ls_r", 2.0 * SC.HEIGHT + 1.0)):
        g = {k: np.array(x) for k, x in f.items()}
        g[key][1, 1] = v
        with pytest.raises(slam_map.PlbaError):
            slam_map.stereo_cpu([g], p)
    with pytest.raises(slam_map.PlbaError):
        slam_map.stereo_cpu([f], dict(p, width=0))
