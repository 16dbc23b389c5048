"""The case table of tests/test_gpu_history.py: which call dirties a handle (D) before which probe (P), as plain data.

A call is a dict.  `kind` says what runs it (test_gpu_history._run):
  velocity  a velocity call through the handle's own forward: `seeds` one frame-pair seed per pair, `goal` "own" (one goal frame
            per pair), "shared" (des_shared) or "cached" (set_goal first, I_des = None), `frames` "synth" (synth.frame_pair) or
            "noise" (saturated noise), `geometry` None (S x S) or the camera frame's (h, w), `mode` / `num_pairs` / `order_seed`
            the selection, `entry` "dev", "host" or "reselect" (a host call, then vitvs_reselect with another order), `in_flight`
            the plan hint, `updates` how many times it runs (the seeds move on each time), `options` = (robust_law, subpatch,
            interaction), `depth` False: no depth image, `select_cells` the option of that name (the image cells per side of BEST)
  forward   a forward-only call: `op` forward_tokens, descriptors, binned, facet:<name>, saliency, correspond or refine
  law       vitvs_servo_from_nn_dev on planted tables: `grid`, `table_seed`, `mode`, `num_pairs`, `pick` (what the selection is made
            of: mutual, repeat1, repeat2, few, no_mutual, all_mutual, same_image), `depth`, `mutual` how many tokens of the planted
            tables are mutual nearest neighbours (None: the 2 T / 3 planted ones and those a random matrix adds), `select_cells`
  follow    a follow-on law: `law` rig, rig_robust, pose, pose_rig or homography with `n_iter`, behind `camera` (a velocity call);
            `consensus` hypotheses drawn from `seed` in front of the pose and the homography law (0: none)
  roll      the roll search: `seed` the frame pair, `turn` quarter turns applied to its current frame, `goal` "own", "cached"
            (set_goal first, I_des = None) or "cached_keep" (I_des = None on whatever goal the handle holds), `mode` / `num_pairs` /
            `order_seed` the selection, `entry` "dev" or "host", `winner` what the search must pick for the row to be what it says:
            "nonzero" (the default with a turn), "zero" (the default without) or "any"; `at_goal` the current frame IS the goal frame
            (the same-image shortcut, the one place where the law reads the flag `rolled` the search leaves)
  seq       `calls` one after the other
`ROWS` are (name, D, P, axis).  `extent(call, axis)` is the one number the axis compares: D's exceeds P's, or for an axis named
"<axis>-reverse" P's exceeds D's; tests/test_history_cases_host.py holds the table to that without a GPU."""

SELECT = {"explicit": 0, "order": 1, "dense": 2, "best": 3}
TOKENS = 196                # of the tiny model (a 14 x 14 grid)
OFF = (0, 0, 0)
ALL_ON = (4, 1, 2)
LDS_ROWS = 128              # L lives in LDS up to this many rows (2 per feature pair), in the global workspace beyond


def velocity(seeds, goal="own", frames="synth", geometry=None, mode="order", num_pairs=24, order_seed=11, entry="dev", in_flight=None,
             updates=1, options=OFF, depth=True, select_cells=4):
    return dict(kind="velocity", seeds=tuple(seeds), goal=goal, frames=frames, geometry=geometry, mode=mode, num_pairs=num_pairs,
                order_seed=order_seed, entry=entry, in_flight=in_flight, updates=updates, options=tuple(options), depth=depth,
                select_cells=select_cells)


def forward(op, seeds):
    return dict(kind="forward", op=op, seeds=tuple(seeds))


def law(table_seed, pick="mutual", mode="explicit", num_pairs=24, grid=17, depth=True, mutual=None, select_cells=4):
    return dict(kind="law", table_seed=table_seed, pick=pick, mode=mode, num_pairs=num_pairs, grid=grid, depth=depth, mutual=mutual,
                select_cells=select_cells)


def follow(name, n_iter, camera, consensus=0, seed=0):
    return dict(kind="follow", law=name, n_iter=n_iter, camera=camera, consensus=consensus, seed=seed)


def roll(seed, turn=1, goal="own", mode="order", num_pairs=24, order_seed=11, entry="dev", winner=None, at_goal=False):
    return dict(kind="roll", seed=seed, turn=turn, goal=goal, mode=mode, num_pairs=num_pairs, order_seed=order_seed, entry=entry,
                winner=winner or ("nonzero" if turn else "zero"), select_cells=4, at_goal=at_goal)


def seq(*calls):
    return dict(kind="seq", calls=list(calls))


# ---------------------------------------------------------------------------------------------- what an axis compares
STATUS_RANK = {"mutual": 0, "same_image": 1, "few": 2, "no_mutual": 2, "all_mutual": 2, "no_depth": 3}
SOLVER_RANK = {"mutual": 0, "repeat1": 1, "repeat2": 2}          # LDL^T, Jacobi (rank 2), Jacobi near the sweep cap (rank 4)
ENTRY_RANK = {"dev": 0, "host": 1, "reselect": 2}


def _leaves(call):
    if call["kind"] == "seq":
        return [x for c in call["calls"] for x in _leaves(c)]
    if call["kind"] == "follow":
        return _leaves(call["camera"]) + [call]
    return [call]


def _law_rows(c):
    """Rows of L a law call builds (an upper bound for DENSE: every token mutual)."""
    if c["kind"] == "law":
        return 2 * (c["grid"] ** 2 if c["mode"] == "dense" else c["num_pairs"])
    return 2 * (196 if c["mode"] == "dense" else c["num_pairs"])


def _mutual(c):
    """Planted mutual tokens of a law call's tables (0 for the picks that plant none, and for calls through the forward)."""
    if c["kind"] != "law" or c["pick"] in ("no_mutual", "all_mutual"):
        return 0
    t = c["grid"] ** 2
    return (2 * t) // 3 if c["mutual"] is None else c["mutual"]


def _order_tokens(c):
    """Tokens the visiting order of a BEST call covers: n_pairs * T."""
    if c["kind"] == "law":
        return c["grid"] ** 2
    return (len(c["seeds"]) if c["kind"] == "velocity" else 1) * TOKENS


def _camera_pairs(cam):
    return len(cam["seeds"]) if cam["kind"] == "velocity" else 1


def extent(call, axis):
    leaves = _leaves(call)
    vel = [c for c in leaves if c["kind"] == "velocity"]
    rolls = [c for c in leaves if c["kind"] == "roll"]
    if axis == "select":         # does a leaf run BEST; then the tokens its order covers, the mutual ones among them, the cells per side
        best = [c for c in leaves if c.get("mode") == "best"]
        return max([(1, _order_tokens(c), _mutual(c), c["select_cells"]) for c in best] + [(0, 0, 0, 0)])
    if axis == "consensus":      # hypotheses, re-weightings, rows of the camera law, pairs (then the seed: another draw of as many)
        f = [c for c in leaves if c["kind"] == "follow"]
        return max([(c["consensus"], c["n_iter"], _law_rows(c["camera"]), _camera_pairs(c["camera"]), c["seed"]) for c in f] + [(0, 0, 0, 0, 0)])
    if axis == "roll":           # a roll call present, the winner is not 0
        return max([(1, int(c["winner"] == "nonzero")) for c in rolls] + [(0, 0)])
    if axis == "pairs":          # images through one forward: goal frames + current frames (a forward-only call: both frames of each seed)
        goals = {"own": lambda n: n, "shared": lambda n: 1, "cached": lambda n: 0, "cached_keep": lambda n: 0}
        return max([len(c["seeds"]) + goals[c["goal"]](len(c["seeds"])) for c in vel] +
                   [2 * len(c["seeds"]) for c in leaves if c["kind"] == "forward"])
    if axis == "in_flight":
        return max(c["in_flight"] or 1 for c in vel)
    if axis == "geometry":       # bytes of one staged frame
        return max((c["geometry"] or (224, 224))[0] * (c["geometry"] or (224, 224))[1] * 3 for c in vel)
    if axis == "entry":          # 0: the probe's own entry point; anything else is another one
        return max([ENTRY_RANK[c["entry"]] for c in vel] + [3 for c in leaves if c["kind"] in ("forward", "law", "roll")])
    if axis == "graph":          # work the eager calls put through the workspaces a replay reads
        return sum(len(c["seeds"]) * c["num_pairs"] * c["updates"] for c in vel) + sum(4 * c["num_pairs"] for c in rolls)
    if axis == "rows":           # which side of the LDS edge L lives on, then the rows
        rows = max(_law_rows(c) for c in leaves if c["kind"] in ("law", "velocity"))
        return (rows > LDS_ROWS, rows)
    if axis == "solver":
        return max(SOLVER_RANK[c["pick"]] for c in leaves if c["kind"] == "law")
    if axis == "status":
        return max(3 if not c["depth"] else STATUS_RANK[c["pick"]] for c in leaves if c["kind"] == "law")
    if axis == "options":        # options that are on
        return max(sum(1 for o in c["options"] if o) for c in vel)
    if axis == "follow":         # the follow-on law's re-weightings, then the rows of the camera law it reads
        f = [c for c in leaves if c["kind"] == "follow"]
        return (max(c["n_iter"] for c in f), max(_law_rows(c["camera"]) for c in f), max(len(c["camera"]["seeds"]) for c in f))
    if axis == "first_use":      # velocity calls the handle has run before the law's first call
        return sum(c["updates"] for c in vel)
    raise KeyError(axis)


def inputs(call):
    """What a call's data is drawn from: frame seeds and table seeds."""
    out = set()
    for c in _leaves(call):
        if c["kind"] in ("velocity", "forward"):
            out |= {("frame", s) for s in c["seeds"]}
        elif c["kind"] == "roll":
            out.add(("frame", c["seed"]))
        elif c["kind"] == "law":
            out.add(("table", c["table_seed"]))
    return out


# ---------------------------------------------------------------------------------------------- the calls
PROBE_SEEDS = (20250705, 20250715, 20250738, 20250751)
DIRT_SEEDS = (31, 32, 33, 34)

P1 = velocity(PROBE_SEEDS[:1])                                            # one pair, ORDER, 24 feature pairs
P4 = velocity(PROBE_SEEDS)
P4_SHARED = velocity(PROBE_SEEDS, goal="shared")
P1_CACHED = velocity(PROBE_SEEDS[:1], goal="cached")
D4 = velocity(DIRT_SEEDS, order_seed=12, num_pairs=48)
D4_SHARED = velocity(DIRT_SEEDS, goal="shared", order_seed=12, num_pairs=48)
D4_NOISE = velocity(DIRT_SEEDS, frames="noise", order_seed=12, num_pairs=48)
D1 = velocity(DIRT_SEEDS[:1], order_seed=12, num_pairs=48)
CAMERA = (480, 640)
# The roll search on the tiny weights: the current frame of every seed of DIRT_SEEDS and PROBE_SEEDS turned by m = 1, 2, 3 quarter
# turns is won by candidate 4 - m, unturned by candidate 0, in the four precisions (measured; the runner asserts the class)
ROLL_DIRT, ROLL_PROBE = DIRT_SEEDS[0], PROBE_SEEDS[0]
ROLL_D = roll(ROLL_DIRT, turn=1, order_seed=12, num_pairs=48)                # winner 3
ROLL_P = roll(ROLL_PROBE, turn=2)                                             # winner 2
BEST_D1 = velocity(DIRT_SEEDS[:1], mode="best", num_pairs=48)
BEST_P1 = velocity(PROBE_SEEDS[:1], mode="best")
CAM_ONE = velocity(PROBE_SEEDS[:1], num_pairs=48)
CAM_ONE_DIRT = velocity(DIRT_SEEDS[:1], order_seed=12, num_pairs=48)

ROWS = [
    # 1. pairs per call
    ("four_pairs_then_one", D4, P1, "pairs"),
    ("four_noise_pairs_then_one", D4_NOISE, P1, "pairs"),
    ("four_goals_then_four_pairs_one_goal", D4, P4_SHARED, "pairs"),
    ("one_goal_then_four_goals", D4_SHARED, P4, "pairs-reverse"),
    ("one_pair_then_four", D1, P4, "pairs-reverse"),
    ("four_pairs_then_forward_tokens", D4, forward("forward_tokens", PROBE_SEEDS[:1]), "pairs"),
    ("four_pairs_then_descriptors", D4, forward("descriptors", PROBE_SEEDS[:1]), "pairs"),
    ("four_pairs_then_binned_key_facet", D4, forward("binned:key", PROBE_SEEDS[:1]), "pairs"),
    ("four_pairs_then_value_facet", D4, forward("facet:value", PROBE_SEEDS[:1]), "pairs"),
    ("four_pairs_then_correspond", D4, forward("correspond", PROBE_SEEDS[:1]), "pairs"),
    ("four_pairs_then_refine", D4, forward("refine", PROBE_SEEDS[:1]), "pairs"),
    # 2. the plan hint on a live handle
    ("in_flight_3_then_1", velocity(DIRT_SEEDS[:1], in_flight=3, updates=3, order_seed=12), velocity(PROBE_SEEDS[:1], in_flight=1),
     "in_flight"),
    ("in_flight_3_four_pairs_then_1", velocity(DIRT_SEEDS, in_flight=3, updates=3, order_seed=12), velocity(PROBE_SEEDS[:1], in_flight=1),
     "in_flight"),
    ("in_flight_1_then_3", velocity(DIRT_SEEDS, in_flight=1, updates=3, order_seed=12), velocity(PROBE_SEEDS[:1], in_flight=3),
     "in_flight-reverse"),
    # 3. frame geometry
    ("camera_frames_then_square", velocity(DIRT_SEEDS[:2], frames="noise", geometry=CAMERA, updates=2, order_seed=12), P1, "geometry"),
    ("camera_frames_host_then_square", velocity(DIRT_SEEDS[:2], frames="noise", geometry=CAMERA, entry="host", order_seed=12), P1,
     "geometry"),
    ("square_then_camera_frames", D4, velocity(PROBE_SEEDS[:1], frames="noise", geometry=CAMERA), "geometry-reverse"),
    ("camera_frames_then_cached_square_goal", velocity(DIRT_SEEDS[:2], frames="noise", geometry=CAMERA, order_seed=12), P1_CACHED,
     "geometry"),
    ("square_then_cached_camera_goal", D4, velocity(PROBE_SEEDS[:1], frames="noise", geometry=CAMERA, goal="cached"), "geometry-reverse"),
    # 5. graph replay (the probe is captured, D runs eagerly between capture and replay)
    ("eager_four_pairs_between_replays", velocity(DIRT_SEEDS, frames="noise", order_seed=12, num_pairs=130, updates=2), P1, "graph"),
    ("eager_dense_between_replays", velocity(DIRT_SEEDS[:3], mode="dense", order_seed=12, updates=2), P1, "graph"),
    # 6. rows, and where L lives
    ("dense_global_L_then_8_pairs", law(901, mode="dense"), law(902, mode="order", num_pairs=8), "rows"),
    ("8_pairs_then_dense_global_L", law(903, mode="order", num_pairs=8), law(904, mode="dense"), "rows-reverse"),
    ("130_pairs_then_64", law(905, num_pairs=130), law(906, num_pairs=64), "rows"),
    # 7. solver path
    ("jacobi_one_token_then_ldlt", law(911, pick="repeat1"), law(912), "solver"),
    ("jacobi_two_tokens_then_ldlt", law(913, pick="repeat2"), law(912), "solver"),
    ("jacobi_global_copy_then_ldlt", law(914, pick="repeat2", num_pairs=80), law(915, num_pairs=80), "solver"),
    ("ldlt_then_jacobi_two_tokens", law(916), law(917, pick="repeat2"), "solver-reverse"),
    ("ldlt_then_jacobi_global_copy", law(918, num_pairs=80), law(919, pick="repeat1", num_pairs=80), "solver-reverse"),
    # 8. statuses
    ("too_few_then_normal", law(921, pick="few"), law(922, mode="order"), "status"),
    ("no_correspondence_then_normal", seq(law(923, pick="no_mutual", mode="order"), law(923, pick="all_mutual", mode="order")),
     law(922, mode="order"), "status"),
    ("no_depth_then_normal", law(924, mode="dense", depth=False), law(922, mode="order"), "status"),
    ("same_image_then_normal", law(925, pick="same_image", mode="order"), law(922, mode="order"), "status"),
    ("normal_then_too_few", law(926, mode="dense"), law(927, pick="few"), "status-reverse"),
    ("normal_then_no_correspondence", law(926, mode="dense"), law(928, pick="no_mutual", mode="order"), "status-reverse"),
    ("normal_then_every_token_mutual", law(926, mode="dense"), law(928, pick="all_mutual", mode="order"), "status-reverse"),
    ("normal_then_no_depth", law(926, mode="dense"), law(929, mode="dense", depth=False), "status-reverse"),
    ("normal_then_same_image", law(926, mode="dense"), law(930, pick="same_image", mode="order"), "status-reverse"),
    # 9. options
    ("all_options_then_none", velocity(DIRT_SEEDS[:2], options=ALL_ON, order_seed=12, num_pairs=48), P1, "options"),
    ("robust_law_then_none", velocity(DIRT_SEEDS[:2], options=(4, 0, 0), order_seed=12, num_pairs=48), P1, "options"),
    ("subpatch_then_none", velocity(DIRT_SEEDS[:2], options=(0, 1, 0), order_seed=12, num_pairs=48), P1, "options"),
    ("interaction_then_none", velocity(DIRT_SEEDS[:2], options=(0, 0, 2), order_seed=12, num_pairs=48), P1, "options"),
    ("none_then_all_options", D4, velocity(PROBE_SEEDS[:1], options=ALL_ON), "options-reverse"),
    ("none_then_desired_interaction", D4, velocity(PROBE_SEEDS[:1], options=(0, 0, 1)), "options-reverse"),
    # 12. selection BEST: one more launch writes the visiting order of n_pairs * T tokens into a workspace the law then reads
    ("best_four_noise_pairs_then_order", velocity(DIRT_SEEDS, frames="noise", mode="best", num_pairs=48), P1, "select"),
    ("order_then_best_four_pairs", D1, velocity(PROBE_SEEDS, mode="best", num_pairs=48), "select-reverse"),
    ("best_4_cells_then_1", BEST_D1, velocity(PROBE_SEEDS[:1], mode="best", select_cells=1), "select"),
    ("best_1_cell_then_4", velocity(DIRT_SEEDS[:1], mode="best", num_pairs=48, select_cells=1), BEST_P1, "select-reverse"),
    ("best_long_order_then_short", law(961, mode="best"), law(962, mode="best", mutual=12, num_pairs=24), "select"),
    ("best_short_order_then_long", law(963, mode="best", mutual=12, num_pairs=24), law(964, mode="best"), "select-reverse"),
    ("best_no_correspondence_then_normal", law(965, pick="no_mutual", mode="best"), law(966, mode="best"), "select-reverse"),
    ("eager_four_pairs_between_best_replays", velocity(DIRT_SEEDS, frames="noise", order_seed=12, num_pairs=130), BEST_P1, "graph"),
    # 13. the roll search: five images through the forward, the keys of four pairs, pair 0's rewritten in place, the flag `rolled`
    ("roll_then_one_pair", ROLL_D, P1, "roll"),
    ("roll_then_four_pairs_four_goals", ROLL_D, P4, "roll"),
    ("four_pairs_then_roll", D4, ROLL_P, "roll-reverse"),
    ("four_pairs_one_goal_then_roll_host", D4_SHARED, dict(ROLL_P, entry="host"), "roll-reverse"),
    ("roll_winner_3_then_winner_0", ROLL_D, roll(ROLL_PROBE, turn=0), "roll"),
    ("roll_winner_3_then_at_the_goal", ROLL_D, roll(ROLL_PROBE, turn=0, at_goal=True), "roll"),
    ("roll_then_pose_consensus", ROLL_D, follow("pose", 4, CAM_ONE, consensus=256), "roll"),
    ("pose_consensus_then_roll", seq(CAM_ONE_DIRT, follow("pose", 4, CAM_ONE_DIRT, consensus=256)), ROLL_P, "roll-reverse"),
    ("four_pairs_then_roll_best", D4, roll(ROLL_PROBE, turn=3, mode="best"), "roll-reverse"),
    ("eager_roll_between_replays", ROLL_D, P1, "graph"),
]

# 4. entry points: (name, D, does the goal cached by set_goal survive D?)  The probe is P1_CACHED.
_HOST = dict(order_seed=12, num_pairs=48)
ENTRY_ROWS = [
    ("compute_velocity_host", velocity(DIRT_SEEDS[:1], entry="host", **_HOST), False),          # a velocity call WITH I_des
    ("reselect_host", velocity(DIRT_SEEDS[:1], entry="reselect", goal="cached_keep", **_HOST), True),   # forwards no goal frame
    ("servo_from_nn", law(941, grid=14, mode="dense"), True),                                   # no forward at all
    ("correspond", forward("correspond", DIRT_SEEDS[:1]), False),                               # overwrites the descriptors
    ("extract_saliency_maps", forward("saliency", DIRT_SEEDS[:2]), False),                      # vitvs_extract_*
    ("extract_descriptors_key", forward("binned:key", DIRT_SEEDS[:2]), False),                  # vitvs_extract_*
    ("compute_velocity_host_best", velocity(DIRT_SEEDS[:1], entry="host", mode="best", **_HOST), False),   # WITH I_des, BEST
    ("roll_own_goal", roll(ROLL_DIRT, goal="own", order_seed=12, num_pairs=48), False),          # forwards a goal frame of its own
    # I_des NULL: the four turned copies are matched against the goal the handle holds, which stays (include/vitvs.h); against
    # another pair's goal the search may pick any winner
    ("roll_cached_goal", roll(ROLL_DIRT, goal="cached_keep", order_seed=12, num_pairs=48, winner="any"), True),
]
ROWS += [("entry_" + name, d, P1_CACHED, "entry") for name, d, _ in ENTRY_ROWS]

# 10. follow-on laws: D the law with 4 re-weightings behind a 130-pair call of three cameras, P the plain law behind an 8-pair
# call of two ("rig_robust" with no re-weighting IS the rig law: the two share the handle's block)
FOLLOW_LAWS = ["rig", "rig_robust", "pose", "pose_rig", "homography"]
CAM_BIG = velocity(DIRT_SEEDS[:3], order_seed=12, num_pairs=130)
CAM_SMALL = velocity(PROBE_SEEDS[:2], num_pairs=8)
for _name in FOLLOW_LAWS:
    _big = follow(_name, 0 if _name == "rig" else 4, CAM_BIG)
    _small = follow("rig" if _name == "rig_robust" else _name, 0, CAM_SMALL)
    _small_robust = follow(_name, 0 if _name == "rig" else 4, CAM_SMALL)
    ROWS.append((f"follow_{_name}_big_then_small", _big, _small, "follow"))
    ROWS.append((f"follow_{_name}_small_then_big", _small, _big, "follow-reverse"))
    ROWS.append((f"follow_{_name}_first_use_after_20_updates", velocity(DIRT_SEEDS[:3], order_seed=12, num_pairs=130, updates=20),
                 _small_robust, "first_use"))

# 14. consensus starts of the pose and the homography law: eight consensus cells in front of the usable-row list in the law's
# scratch, another LDS plan; the one scratch block serves no hypotheses, 256 and 4096 (the hypotheses per thread change), one
# pair to three.  "The same camera call" is one of the same shape on other frames: D and P share no input.
CONSENSUS_LAWS = ["pose", "homography"]
CAM_BIG_PROBE = velocity(PROBE_SEEDS[:3], num_pairs=130)
for _name in CONSENSUS_LAWS:
    _many = follow(_name, 4, CAM_BIG, consensus=4096, seed=7)
    _plain = follow(_name, 0, CAM_SMALL)
    ROWS.append((f"consensus_{_name}_4096_then_none", _many, _plain, "consensus"))
    ROWS.append((f"consensus_{_name}_none_then_4096", follow(_name, 0, velocity(DIRT_SEEDS[:2], order_seed=12, num_pairs=8)),
                 follow(_name, 4, CAM_BIG_PROBE, consensus=4096, seed=7), "consensus-reverse"))
    ROWS.append((f"consensus_{_name}_4096_then_256", _many, follow(_name, 4, CAM_BIG_PROBE, consensus=256, seed=7), "consensus"))
    ROWS.append((f"consensus_{_name}_seed_7_then_0", follow(_name, 4, CAM_BIG, consensus=256, seed=7),
                 follow(_name, 4, CAM_BIG_PROBE, consensus=256, seed=0), "consensus"))
    ROWS.append((f"consensus_{_name}_first_use_after_20_updates", velocity(DIRT_SEEDS[:3], order_seed=12, num_pairs=130, updates=20),
                 follow(_name, 4, CAM_SMALL, consensus=256, seed=7), "first_use"))

# 11. refused calls between D and P (test_gpu_history._REFUSALS makes them; all are rejected on the host)
REFUSALS = ["num_pairs_above_max_rows", "half_a_geometry", "null_pointer", "robust_iterations_17", "f16x2_saliency"]

# The pool of the long mixed sequence: one tiny handle, max_pairs = 4, max_rows = 196
POOL = [
    ("one_pair", P1),
    ("four_pairs", P4),
    ("four_pairs_one_goal", P4_SHARED),
    ("four_noise_pairs_130", velocity(DIRT_SEEDS, frames="noise", order_seed=12, num_pairs=130)),
    ("dense_two_pairs", velocity(DIRT_SEEDS[:2], mode="dense")),
    ("host_then_reselect", velocity(PROBE_SEEDS[1:3], entry="reselect", order_seed=13)),
    ("cached_goal", P1_CACHED),
    ("camera_frames", velocity(DIRT_SEEDS[2:4], frames="noise", geometry=CAMERA, in_flight=3)),
    ("all_options", velocity(PROBE_SEEDS[2:4], options=ALL_ON, num_pairs=48)),
    ("forward_tokens", forward("forward_tokens", DIRT_SEEDS[:3])),
    ("binned_key_facet", forward("binned:key", PROBE_SEEDS[:2])),
    ("correspond", forward("correspond", PROBE_SEEDS[3:])),
    ("jacobi_law", law(951, pick="repeat2", grid=14)),
    ("too_few_law", law(952, pick="few", grid=14)),
    ("rig_robust", follow("rig_robust", 4, velocity(PROBE_SEEDS[:3], order_seed=14))),
    ("roll_winner_3", ROLL_D),
    ("best_two_pairs", velocity(PROBE_SEEDS[1:3], mode="best", num_pairs=48)),
    ("pose_consensus", follow("pose", 4, velocity(DIRT_SEEDS[:2], order_seed=14, num_pairs=48), consensus=256, seed=7)),
]
