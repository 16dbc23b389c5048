"""Sub-patch refinement of matches (option ``subpatch``) on the CPU: the fp64 reference (tests/refine_ref.py) on
hand-made similarity rows, the displacement study that decides whether the idea works on this project's fixtures at all, and
the plumbing of the option (parameters, configuration mapping, C prototypes).  No GPU."""
import numpy as np
import pytest

import vitvs_amd  # noqa: F401
from vitvs_amd import _lib, config

import refine_ref as rr

G = 5                        # grid of the hand-made cases
CENTRE = 2 * G + 2           # token (2, 2): an interior token


def _row_case(centre_vals, j=CENTRE, g=G):
    """One goal token (row 0 of S) matched to ``j``; ``centre_vals`` = {token: similarity}, everything else -1."""
    S = np.full((g * g, g * g), -1.0)
    for tok, val in centre_vals.items():
        S[0, tok] = val
    nn1 = np.zeros(g * g, np.int64)
    nn1[0] = j
    return rr.offsets_from_similarity(S, nn1, g)[0]


def test_symmetric_neighbours_give_zero():
    dr, dc = _row_case({CENTRE: 0.9, CENTRE - 1: 0.5, CENTRE + 1: 0.5, CENTRE - G: 0.3, CENTRE + G: 0.3})
    assert dr == 0.0 and dc == 0.0


def test_known_parabola_gives_its_vertex():
    # S(x) = 0.9 - 0.2 (x - 0.3)^2 along the columns, 0.9 - 0.1 (y + 0.25)^2 along the rows (same peak value: one matrix entry)
    f = lambda x: 0.9 - 0.2 * (x - 0.3) ** 2 + 0.2 * 0.09       # noqa: E731   f(0) = 0.9
    h = lambda y: 0.9 - 0.1 * (y + 0.25) ** 2 + 0.1 * 0.0625    # noqa: E731   h(0) = 0.9
    dr, dc = _row_case({CENTRE: 0.9, CENTRE - 1: f(-1), CENTRE + 1: f(1), CENTRE - G: h(-1), CENTRE + G: h(1)})
    assert abs(dc - 0.3) <= 1e-12 and abs(dr + 0.25) <= 1e-12


@pytest.mark.parametrize("j", [0, 2, G - 1, 2 * G, 2 * G + G - 1, G * G - 1, G * G - 3])
def test_border_tokens_have_no_offset_across_the_border(j):
    r, c = divmod(j, G)
    vals = {j: 0.9}
    for nb, v in ((j - 1, 0.8), (j + 1, 0.2), (j - G, 0.7), (j + G, 0.1)):
        if 0 <= nb < G * G:
            vals[nb] = v
    dr, dc = _row_case(vals, j=j)
    assert (dc == 0.0) == (c in (0, G - 1)) and (dr == 0.0) == (r in (0, G - 1))


def test_flat_row_gives_zero_not_nan():
    dr, dc = _row_case({CENTRE: 0.5, CENTRE - 1: 0.5, CENTRE + 1: 0.5, CENTRE - G: 0.5, CENTRE + G: 0.5})
    assert dr == 0.0 and dc == 0.0


def test_non_negative_denominator_gives_zero():
    # the centre is not the maximum (a rounding tie broken the other way): den = a - 2 m + p >= 0
    dr, dc = _row_case({CENTRE: 0.5, CENTRE - 1: 0.7, CENTRE + 1: 0.4, CENTRE - G: 0.5, CENTRE + G: 0.5 + 1e-9})
    assert dr == 0.0 and dc == 0.0


def test_result_is_always_within_half_a_pitch():
    rng = np.random.default_rng(5)
    g = 9
    S = rng.uniform(-1, 1, size=(g * g, g * g))
    for nn1 in (S.argmax(1), rng.integers(0, g * g, size=g * g)):       # true maxima, and arbitrary tokens (den of any sign)
        off = rr.offsets_from_similarity(S, nn1, g)
        assert np.all(np.isfinite(off)) and np.all(np.abs(off) <= 0.5)
    # near-ties push the raw vertex far outside: the clamp holds it
    off = rr.parabola(np.array([0.5 + 1e-13]), np.array([0.5]), np.array([0.5 - 2e-13]))[0]
    assert np.all(np.abs(off) <= 0.5)


def test_refined_pixels_with_zero_offsets_are_the_patch_centres_of_the_law():
    import torch
    from oracle import servo_ref as sr
    for img, g in ((224, 14), (308, 22), (518, 37)):
        ids = np.arange(g * g)
        pts = sr.patch_centres(torch.from_numpy(np.stack([ids // g, ids % g], 1)), img, g)
        uv, _ = sr.calculate_uv(pts, pts, len(ids), 640, 480, img)
        assert np.array_equal(rr.refined_pixels(ids, np.zeros((g * g, 2)), img, g, 640, 480), np.asarray(uv))


def test_displacement_study_refinement_lowers_the_error():
    """The fixture of tests/test_gpu_loop.py (vits16_224, synthetic weights seed 0, synth.texture(128, 11) over 1.6 m at 0.61 m),
    goal view against views from a camera moved sideways by (0.1, 0.3), (0.2, 0.4), (0.3, 0.1), (0.4, 0.2), (0.5, 0.25) patch
    pitches in (u, v); mutual matches within one pitch of the truth; errors in pitches.  Measured with the fp64 reference:

        shift (u, v)   mutual  near   rms plain  rms refined   |mean error| plain  refined
        (0.1, 0.3)       195    195     0.2236     0.2246          0.3162          0.1499
        (0.2, 0.4)       154    153     0.3214     0.2745          0.4182          0.2440
        (0.3, 0.1)       182    181     0.2236     0.2492          0.3162          0.1879
        (0.4, 0.2)       135    130     0.3486     0.3203          0.3757          0.2418
        (0.5, 0.25)       90     80     0.4330     0.3536          0.2151          0.1688
        all                             0.2975     0.2751  (x 0.925)   0.3283      0.1985  (x 0.605, mean of the rows)

    With the synthetic (untrained) weights the offset of a single match scatters by ~0.2 pitch even between identical views (the
    similarity of a goal token to the two neighbours of its match is not symmetric), so per match the refinement gains little:
    7.5 % overall, and at the two smallest shifts nothing.  What it removes is the COMMON error of the matches — all patch
    centres are wrong by the same sub-patch shift, and the scatter averages out over the features of a least-squares law: the
    mean error falls by 40 %.  Bars: half-way between the measured ratio and 1 (0.96 and 0.80); a different BLAS summation order
    moves a similarity by ~1e-7 and an offset by ~1e-6 of a pitch, far below either margin."""
    d = rr.displacement_study()
    for row in d["rows"]:
        print("shift ({fu}, {fv}): mutual {mutual}, near {near}, rms {rms_plain:.4f} -> {rms_refined:.4f}, "
              "|mean error| {bias_plain:.4f} -> {bias_refined:.4f}".format(**row))
    print(f"all: rms {d['rms_plain']:.4f} -> {d['rms_refined']:.4f} (x {d['rms_refined'] / d['rms_plain']:.3f}), "
          f"|mean error| {d['bias_plain']:.4f} -> {d['bias_refined']:.4f} (x {d['bias_refined'] / d['bias_plain']:.3f})")
    assert all(row["near"] >= 40 for row in d["rows"])
    assert d["rms_refined"] <= 0.96 * d["rms_plain"]
    assert d["bias_refined"] <= 0.80 * d["bias_plain"]
    assert all(row["bias_refined"] < row["bias_plain"] for row in d["rows"])


# ----------------------------------------------------------------------------- plumbing
def test_servo_params_carry_the_option():
    assert config.ServoParams().subpatch is False
    p = config.ServoParams(subpatch=True)
    assert p.subpatch is True and p.replace(subpatch=False).subpatch is False


def _reference_mapping():
    return {"u_max": 640, "v_max": 480, "f_x": 500.0, "f_y": 500.0, "lambda_": 0.03, "min_error": 1, "max_error": 2,
            "num_pairs": 24, "thresh_filter_keypoints": 0.1, "dino_input_size": 308, "use_feature_binning": True,
            "num_samples": 1, "num_circles": 1, "circle_radius_aug": 1, "velocity_convergence_threshold": 0.1,
            "velocity_threshold_translation": 0.1, "velocity_threshold_rotation": 0.1, "error_threshold_ratio": 0.1,
            "error_threshold_absolute_translation": 0.1, "error_threshold_absolute_rotation": 0.1, "min_iterations": 1,
            "max_iterations": 10, "image_path": "goal.png"}


def test_load_reference_config_takes_the_key_when_present():
    m = _reference_mapping()
    rc = config.load_reference_config(m)
    assert rc.servo.subpatch is False and "subpatch" not in rc.extras
    m["subpatch"] = True
    rc = config.load_reference_config(m)
    assert rc.servo.subpatch is True and "subpatch" not in rc.extras


def test_prototypes_present():
    for name in ("vitvs_refine_dev", "vitvs_servo_from_nn_ex_dev", "vitvs_last_offsets"):
        assert name in _lib.PROTOTYPES
    assert _lib.ABI_VERSION == 2
    lib = _lib.load()                       # binds every prototype: raises when the library lacks one
    assert lib.vitvs_refine_dev is not None


@pytest.mark.parametrize("kind", ["smooth", "random"])
@pytest.mark.parametrize("T", rr.SEAM_TOKENS)
def test_descriptor_cases_of_the_device_tests_are_well_conditioned(T, kind):
    """The inputs of tests/test_gpu_refine.py on the reference alone: at most 5 % of a case's parabolas have an fp64 |den| below
    1e-4, and the error of an fp32 numpy evaluation of the same formula against fp64 (the device test's bar is 4 x that, per
    case).  Measured (largest |delta_fp32 - delta_fp64| over the parabolas with |den| >= 1e-4, Dp = 384 / 768 / 1024 / 3456):
        smooth  T =  196: 2.4e-06 1.8e-06 1.3e-06 6.9e-07     random  T =  196: 8.4e-07 5.1e-07 4.0e-07 5.6e-07
        smooth  T =  484: 2.1e-06 1.4e-06 1.2e-06 8.1e-07     random  T =  484: 1.2e-06 4.2e-07 5.0e-07 5.0e-07
        smooth  T = 1369: 2.6e-06 1.4e-06 1.4e-06 9.4e-07     random  T = 1369: 1.1e-06 5.2e-07 5.4e-07 3.6e-07
    (median |den| 0.36 .. 0.39 smooth, 0.09 .. 0.33 random); no case has a parabola below the 1e-4 line."""
    g = int(round(np.sqrt(T)))
    for Dp in rr.SEAM_WIDTHS:
        d1, d2 = rr.descriptor_case(T, Dp, kind)
        S = rr.cosine_similarity(d1, d2)
        nn1 = S.argmax(1)
        ref, den = rr.offsets_from_similarity(S, nn1, g, with_den=True)
        f32 = rr.offsets(d1, d2, nn1, g, dtype=np.float32)
        big, small, share = rr.offset_errors(f32, ref, den)
        print(f"{kind} T={T} Dp={Dp}: fp32 numpy against fp64 {big:.2e} (|den| >= 1e-4), {small:.2e} below, share below {share:.4f}, "
              f"median |den| {np.nanmedian(np.abs(den)):.3f}")
        assert share <= rr.SMALL_DEN_SHARE and small <= 0.5 and np.all(np.abs(ref) <= 0.5)
