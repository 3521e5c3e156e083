"""The session sequences without a GPU (tests/session_cases.py; tests/test_session_gpu.py plays them on the device): generation is
deterministic, every circuit holds every ordered pair of kinds exactly once and cutting loses none, camera and shape steps change the
state; on the oracles alone the visited states are not vacuous (hit shares, changed shares), the caps hold (refusals, accepting
temporal steps, a temporal step on an older frame and a motion step with camera and shape both changed in every circuit), and the
model, driven through the chains of motion_cases.py and temporal_cases.py, gives exactly their states, references and histories.
The edit seeds: their caps (class crossings by direction and cause, frames, clones, histories and mattes around them), the shares by
which an edit changes the oracle's planes and mattes differ, and that planes and mattes of an edited look are those of a scene built
with the look's fields from the start.
The post seeds: how often each situation of session_cases.POST_FACTS occurs, the share of the pixels in which the clamped oracle differs
from the unclamped one where a history is live, the gather shares of the blurs and that they change their frames, and that the model
gives what the three features' own GPU tests compute from their oracles for their hand-written chains."""
import collections

import numpy as np
import pytest

import ctypes as C

import geometry_cases as GC
import motion_cases as MC
import motion_oracle as MO
import oracle_lib as O
import sample_window_cases as WC
import session_cases as SC
import temporal_cases as TC
import temporal_oracle as TO
from opencl_render_amd import raytrace as R

F32 = np.float32


def circuits():
    return [(name, seed) for name, spec in SC.SCENES.items() for seed in spec["circuits"] + spec["wide_circuits"] + spec.get("edit_circuits", ())
            + spec.get("post_circuits", ())]


def every_sequence():
    return [(name, seed, part, SC.part_of(name, seed, part)) for name, seed, part in SC.all_parts()]


# ---- generation -----------------------------------------------------------------------------------------------------------------------
def test_generation_is_deterministic():
    first = {(n, s, p): q for n, s, p, q in every_sequence()}
    SC._sequences.clear()
    again = {(n, s, p): q for n, s, p, q in every_sequence()}
    assert first == again and len(first) == len(SC.all_parts())
    for wide, counts in ((False, SC.COUNTS), (True, SC.COUNTS_WIDE)):  # the seeds drawn before the wide alphabet existed are what they were
        mine = [q for (n, s, p), q in first.items() if s in SC.seeds_of(n, wide)]
        assert dict(sequences=len(mine), steps=sum(len(q["steps"]) for q in mine)) == counts, f"the draw changed (wide: {wide}): measure again"
    mine = [q for (n, s, p), q in first.items() if s in SC.edit_seeds(n)]
    assert dict(sequences=len(mine), steps=sum(len(q["steps"]) for q in mine)) == SC.COUNTS_EDIT, "the draw of the edit seeds changed: measure again"
    mine = [q for (n, s, p), q in first.items() if s in SC.post_seeds(n)]
    assert dict(sequences=len(mine), steps=sum(len(q["steps"]) for q in mine)) == SC.COUNTS_POST, "the draw of the post seeds changed: measure again"


@pytest.mark.parametrize("name, seed", circuits())
def test_a_circuit_holds_every_ordered_pair_once_and_cutting_loses_none(name, seed):
    parts = SC.sequences(name, seed)
    kinds, end = [], ("home", "home")
    for i, q in enumerate(parts):
        ks = [k for k, _ in q["steps"]]
        assert 2 <= len(ks) <= SC.SCENES[name]["cut"] <= SC.CUT and q["start"] == end
        if i:
            assert ks[0] == kinds[-1], "a sequence does not start with the kind the one before ended in"
            ks = ks[1:]
        kinds += ks
        s = SC.lite_of(name, seed, q["start"])
        for step in q["steps"]:
            s.advance(step)
        end = (s.pose, s.shape)
    alphabet = SC.kinds_of(name, seed)
    K = len(alphabet)
    assert K == (25 if seed in SC.SCENES[name].get("edit_circuits", ()) else 22 if seed in SC.SCENES[name].get("post_circuits", ())
                 else 19 if seed in SC.SCENES[name]["wide_circuits"] else 17)
    assert len(kinds) == K * K + 1 and kinds[0] == kinds[-1]
    pairs = collections.Counter(zip(kinds, kinds[1:]))
    assert len(pairs) == K * K and set(pairs.values()) == {1} and set(k for k, _ in pairs) == set(alphabet)
    within = collections.Counter(p for q in parts for p in zip([k for k, _ in q["steps"]], [k for k, _ in q["steps"]][1:]))
    assert within == pairs, "a pair is adjacent in the circuit but in none of its sequences"


def test_camera_and_shape_steps_change_the_state_and_refusals_stay_rare():
    for name, seed, part, q in every_sequence():
        S = SC.SCENES[name]["samples"]
        s, refused = SC.lite_of(name, seed, q["start"]), 0
        for kind, arg in q["steps"]:
            assert kind in SC.kinds_of(name, seed)
            if kind in ("lights", "materials", "ids"):  # an edit names a set of the tables and always changes the look
                assert s.after((kind, arg)) != s.look, (name, seed, part, kind, arg)
                L, M, (variant, modulus) = s.after((kind, arg))
                assert L in SC.LIGHT_SETS and M in SC.MATERIAL_SETS and variant in SC.ID_VARIANTS
                assert int(SC.look_ids(name, (variant, modulus)).max()) < SC.look_parts(name)["counts"][M], "an id of the look is out of range"
            if kind == "materials":  # ids come exactly where the resident ones would be out of range, and in some draws otherwise
                assert arg[1] is not None or s.max_id() < SC.look_parts(name)["counts"][arg[0]]
            if kind == "refused_edit":
                assert arg in SC.EDIT_REFUSALS and (arg != "shrink" or s.max_id() >= 1)
            if kind == "mattes":
                what, n, layers, window = arg
                assert what in SC.MATTE_KINDS and n in SC.MATTE_SELECT and layers in SC.MATTE_LAYERS
                if window is not None:
                    p = R.MatteParams(kind=0, total=window[0], first=window[1], samples=window[2], selectCount=0, layers=layers)
                    assert R.lib().rtHipMatteCheck(C.byref(p)) == 0, (window, R.last_error())
            if kind == "window" and arg is not None:
                win = arg[1] if s.refuses((kind, arg)) else arg
                rc = R.lib().rtHipSampleWindowCheck(S, C.byref(R.SampleWindow(*win)))
                if s.refuses((kind, arg)):
                    assert rc == -1 and arg[2] in R.last_error(), (name, seed, part, arg, R.last_error())
                else:
                    assert rc == 0 and win[0] in [S * n for n in SC.WINDOW_SIZES], (name, seed, part, arg, R.last_error())
                    assert not (win[3] and win[1] > 0), "a window that continues is drawn at f = 0 only: it never starts on an undefined buffer"
            if kind == "clamp" and arg is not None:  # a setting of the table, or one that the library's check refuses with the text
                mode, gamma = arg[1] if s.refuses((kind, arg)) else arg
                rc = R.lib().rtHipTemporalClampCheck(C.byref(R.temporal_clamp_params(mode, gamma)))
                if s.refuses((kind, arg)):
                    assert rc == -1 and arg[2] in R.last_error() and (arg[1], arg[2]) in SC.CLAMP_REFUSALS, (name, seed, part, arg, R.last_error())
                else:
                    assert rc == 0 and arg in SC.CLAMP_SETTINGS and arg != s.clamp, (name, seed, part, arg, R.last_error())
            if kind == "clamp" and arg is None:
                assert s.clamp is not None, "the clamp is turned off while it is off"
            if kind == "motion_blur":
                assert R.lib().rtHipMotionBlurCheck(C.byref(R.motion_blur_params(**SC.BC.SCENE_PARAMS[arg]))) == 0, arg
            if kind == "dof":
                assert R.lib().rtHipDepthOfFieldCheck(C.byref(R.dof_params(**SC.DC.SCENE_PARAMS[arg]))) == 0, arg
            if kind in ("camera", "refused_camera"):
                assert arg in SC.POSES and arg != s.pose, (name, seed, part, kind, arg)
            if kind == "shape":
                assert arg in SC.SCENES[name]["shapes"] and arg != s.shape, (name, seed, part, kind, arg)
            if kind == "refused_update":
                assert arg[0] in SC.UPDATE_REFUSALS and arg[1] != s.shape
            refused += bool(s.refuses((kind, arg)))
            s.advance((kind, arg))
        assert refused * 5 <= len(q["steps"]), f"{name} seed {seed} part {part}: {refused} of {len(q['steps'])} steps are refusals"
    for name, spec in SC.SCENES.items():
        for seed in spec["walks"] + spec["wide_walks"] + spec.get("edit_walks", ()) + spec.get("post_walks", ()):
            parts = SC.sequences(name, seed)
            assert sum(len(q["steps"]) for q in parts) == SC.WALK + len(parts) - 1  # (a cut walk repeats the kind it was cut at)
            assert all(len(q["steps"]) <= SC.walk_limit(name, seed) for q in parts) and ("walk_cut" in spec or len(parts) == 1)
            assert all(sum(k == "shape" for k, _ in q["steps"]) <= spec.get("shape_steps", SC.WALK) for q in parts)


# ---- the visited states and the caps, on the oracles alone -------------------------------------------------------------------------------
_played = {}


def played(name):
    """The model alone over every sequence of the scene: {(seed, part): notes}, the visited states in order of first visit, and the
    (state, next state) pairs of its camera and shape steps."""
    if name not in _played:
        w = SC.world(name)
        notes, states, moves = {}, [], set()
        for n, seed, part, q in every_sequence():
            if n != name:
                continue
            s = SC.Session(w, q["start"], edit=SC.is_edit(name, seed), post=SC.is_post(name, seed))
            states.append(s.here())
            for step in q["steps"]:
                before = s.here()
                s.apply(step)
                if s.here() != before:
                    moves.add((before, s.here()))
                    states.append(s.here())
            notes[seed, part] = s.notes
        _played[name] = (notes, list(dict.fromkeys(states)), sorted(moves))
    return _played[name]


@pytest.mark.parametrize("name", list(SC.SCENES))
def test_visited_states_hit_and_consecutive_states_differ(name):
    w = SC.world(name)
    _, states, moves = played(name)
    hits = []
    for st in states:
        hits.append(float((w.trace(*st)[1] != SC.NONE).mean()))
        floor = SC.SCENES[name].get("min_hit", MC.MIN_HIT)
        assert hits[-1] >= floor, f"{name}/{st}: only {hits[-1]:.3f} of the centre rays hit"
    changed = []
    for a, b in moves:
        share = GC.changed_share(w.planes(*a), w.planes(*b))
        if a[0] == b[0] and {a[1], b[1]} <= {"home", "reindex"}:  # the same triangles under other indices (geometry_cases.py: the
            planes_moved = not np.array_equal(w.state(*a).box_min, w.state(*b).box_min)  # planes moved with V, or the frame is the same)
            assert planes_moved or share == 0.0, f"{name}: {a} -> {b}: same planes but another frame"
            continue
        changed.append(share)
        assert share >= GC.MIN_CHANGED, f"{name}: {a} -> {b}: the oracle's planes change in {share:.4f} of the pixels only"
    print(f"{name}: {len(states)} states visited, hit share {min(hits):.3f}..{max(hits):.3f}; {len(moves)} distinct moves, changed share "
          f"{min(changed):.3f}..{max(changed):.3f}")
    assert len(states) >= 12 and states == SC.visited(name)
    assert {p for p, _ in states} == set(SC.POSES) and {n for _, n in states} == set(SC.SCENES[name]["shapes"]), "a pose or shape is never visited"


def test_temporal_and_motion_steps_are_not_vacuous():
    accepting = total = 0
    for name, spec in SC.SCENES.items():
        notes, _, _ = played(name)
        for seed in spec["circuits"]:
            mine = [n for (s, _), ns in notes.items() if s == seed for n in ns]
            assert any(k == "temporal" and stale for k, stale, _ in mine), f"{name} seed {seed}: no temporal step on an older frame"
            assert any(k == "motion" and both for k, both, _ in mine), f"{name} seed {seed}: no motion step with camera and shape both changed"
        for (seed, _), ns in notes.items():
            for k, _, share in ns:
                if k == "temporal" and seed in SC.seeds_of(name, wide=False):  # (the figure of COUNTS; the wide seeds have caps of their own)
                    total += 1
                    accepting += share >= TC.MIN_ACCEPT
    print(f"{accepting} of {total} temporal steps accept history in at least {TC.MIN_ACCEPT} of the pixels")
    assert total >= 30 and accepting * 3 >= total


# ---- the wide seeds: sample windows and the moments history -------------------------------------------------------------------------------------
def wide_notes():
    """[(scene, seed, part, notes)] of the wide seeds' sequences, the model alone."""
    return [(name, seed, part, played(name)[0][seed, part]) for name in SC.SCENES for seed in SC.seeds_of(name, wide=True)
            for part in range(len(SC.sequences(name, seed)))]


def saturated(planes):
    return np.stack([np.asarray(p) for p in planes]) == WC.SATURATED


def test_the_wide_seeds_frames_use_windows_and_continue_from_the_tile_buffer():
    frames, complete, brighter = [], collections.Counter(), 0
    continuing, successive = [], []
    for name, seed, part, notes in wide_notes():
        w = SC.world(name)
        mine = [(info, before, planes) for k, info, (before, planes) in (n for n in notes if n[0] == "frame")]
        frames += [info for info, _, _ in mine]
        for info, before, planes in mine:
            pose, shape = info["state"]
            N, f, D, acc, adv = info["window"]
            if info["complete"]:  # a progressive run that completes leaves the plain N-sample frame, saturation included
                want = O.oracle_render(WC.with_samples(w.state(pose, shape), N), threads=16)
                assert WC.differing(planes, want) == 0, f"{name} seed {seed} part {part}: the completed run of {N} at {info['state']}"
                complete[name, seed] += 1
            if info["continuing"]:
                assert before is not None
                zeros = w.window_planes(pose, shape, N, f, D)
                continuing.append(WC.differing(planes, zeros) / (3 * w.width * w.height))
                if info["kind"] == "overbright":  # the same frame with D = N, onto the same buffer
                    dim = O.oracle_render_window(w.state(pose, shape), N, f, N, onto=before, threads=16)
                    brighter += bool((saturated(planes) & ~saturated(dim)).any())
            else:
                assert WC.differing(planes, w.window_planes(pose, shape, N, f, D)) == 0
        for i, j in SC.successive([info for info, _, _ in mine]):
            successive.append(WC.differing(mine[i][2], mine[j][2]) / (3 * w.width * w.height))
    cont = [f for f in frames if f["continuing"]]
    kinds = collections.Counter(f["kind"] for f in frames)
    print(f"wide seeds: {len(frames)} frames {dict(kinds)}, {len(cont)} continue, {sum(f['moved'] for f in cont)} of them after a camera, shape "
          f"or pipeline step; {sum(complete.values())} progressive runs complete; {brighter} over-bright frames saturate a value their D = N "
          f"frame does not; a continuing frame differs from its window from zeros in {np.mean(continuing):.3f} of the plane values "
          f"({min(continuing):.3f}..{max(continuing):.3f}), successive windows of a sequence in {np.mean(successive):.3f} "
          f"({min(successive):.3f}..{max(successive):.3f} over {len(successive)} pairs)")
    assert 3 * (len(frames) - kinds["default"]) >= len(frames)
    assert 10 * len(cont) >= len(frames)
    assert 2 * sum(f["moved"] for f in cont) >= len(cont)
    for name in SC.SCENES:
        for seed in SC.seeds_of(name, wide=True):
            assert complete[name, seed] >= 1, f"{name} seed {seed}: no progressive run completes"
    assert brighter >= 1
    assert set(kinds) == {"default", "progressive", "sequence", "overbright", "fixed"}
    assert np.mean(continuing) >= 0.5 * SC.WINDOW_SHARES["continuing"] > 0
    assert np.mean(successive) >= 0.5 * SC.WINDOW_SHARES["successive"] > 0


def test_the_wide_seeds_variance_steps_find_stale_and_live_moments():
    steps = []
    for name in SC.SCENES:
        for seed in SC.seeds_of(name, wide=True):
            mine = [info for n, s, _, notes in wide_notes() if (n, s) == (name, seed) for k, info, _ in notes if k == "variance"]
            assert any(v["stale"] for v in mine), f"{name} seed {seed}: no variance step finds stale moments over a live history"
            steps += mine
    warm, live = sum(v["warm"] for v in steps), sum(v["live"] for v in steps)
    print(f"wide seeds: {len(steps)} variance steps, {warm} warm, {sum(v['stale'] for v in steps)} restart over stale moments, {live} go on with live moments")
    assert 3 * warm >= len(steps) and live >= 1


def test_the_scenes_of_the_wide_seeds_take_no_split_logic_rounds():
    """Why no sequence is played a second time under RT_WF_LOGIC_SPLIT=0 (session_cases.SCENES): split rounds exist in the
    opaque-diffuse class only, and both scenes that have wide seeds are of the general class (class_textured_bumped, which has the
    edit seeds, is the scene of the opaque-diffuse class)."""
    wide = [name for name in SC.SCENES if SC.seeds_of(name, wide=True)]
    assert wide == ["mirror_hall", "axis_near_axis_mixed"]
    for name in wide:
        assert R.path_class(SC.world(name).base) == R.PATH_CLASS_GENERAL, name


# ---- the edit seeds: looks, class crossings and mattes ---------------------------------------------------------------------------------------------
EDITED = "class_textured_bumped"


def edit_logs():
    """(frames, events) of the edit seeds' sequences, one list per sequence each, from the light state alone."""
    frames, events = [], []
    for seed in SC.edit_seeds(EDITED):
        for q in SC.sequences(EDITED, seed):
            s = SC.lite_of(EDITED, seed, q["start"])
            for step in q["steps"]:
                s.advance(step)
            frames.append(s.frames)
            events.append(s.log.events)
    return frames, events


def test_the_edit_seeds_cross_the_class_boundary_between_all_other_operations():
    frames, events = edit_logs()
    facts = SC.edit_facts(frames, events)
    print(f"edit seeds: {facts}")
    assert R.path_class(SC.world(EDITED).base) == R.PATH_CLASS_OPAQUE_DIFFUSE
    assert {SC.look_class(EDITED, (L, M, None)) for L in SC.LIGHT_SETS for M in SC.MATERIAL_SETS} == {R.PATH_CLASS_GENERAL, R.PATH_CLASS_OPAQUE_DIFFUSE}
    assert int(SC.look_parts(EDITED)["lights"]["many65"]["light_type"].shape[0]) == 65  # past the logic kernel's 64-light split
    assert facts["edits"] >= 60 and facts["same_look"] == 0, "an edit leaves the look as it was"
    for k in ("lights_to_general", "lights_to_opaque_diffuse", "materials_to_general", "materials_to_opaque_diffuse"):
        assert facts[k] >= 2, k
    for k in ("frames_general_after_camera", "frames_general_after_shape", "frames_opaque_diffuse_after_camera", "frames_opaque_diffuse_after_shape",
              "clones_in_another_class", "frames_on_another_look", "temporal_across", "variance_across", "mattes_triangle", "mattes_material",
              "mattes_group", "mattes_group_after_shape", "mattes_group_after_edit", "mattes_material_after_ids", "mattes_before_frames",
              "mattes_refused"):
        assert facts[k] >= 1, k
    assert 3 * facts["mattes_defaults_other_window"] >= facts["mattes_defaults"] > 0
    assert SC.edit_caps(facts)


def test_the_edit_seeds_histories_cross_the_class_boundary_and_show_it():
    """A temporal and a variance step whose live history holds a frame of another class are counted only under max_history > 1 (at 1
    the answer is the frame itself), and at least one of each blends the history in and gives another answer than over an empty
    history: a history that an edit or a class crossing wiped would fail these steps."""
    _, events = edit_logs()
    logged = collections.Counter(e[0] for part in events for e in part if e[0] in ("temporal", "variance") and e[1])
    notes = [n[1:] for seed in SC.edit_seeds(EDITED) for part in range(len(SC.sequences(EDITED, seed)))
             for n in played(EDITED)[0][seed, part] if n[0] == "across"]
    print(f"edit seeds: steps with a live history across a class change (kind, max_history, share of the pixels that blend the history in, "
          f"share that differs from the answer over an empty history): {[(k, f['cap'], round(f['blended'], 3), round(f['differs'], 3)) for k, f in notes]}")
    assert collections.Counter(k for k, _ in notes) == logged, "the model and the light state disagree on which steps cross"
    assert all(f["cap"] > 1 for _, f in notes)
    for kind in ("temporal", "variance"):
        shown = [f for k, f in notes if k == kind and f["blended"] > 0 and f["differs"] > 0]
        assert shown, f"no {kind} step blends a history across a class change into another answer than over an empty history"
    assert SC.histories_cross(notes)


def test_the_edit_seeds_edits_and_mattes_are_not_vacuous():
    frames, events = edit_logs()
    shares = SC.edit_shares(EDITED, frames)
    pairs, differing = SC.matte_pairs(EDITED, events)
    notes = [n for seed in SC.edit_seeds(EDITED) for part in range(len(SC.sequences(EDITED, seed)))
             for n in played(EDITED)[0][seed, part] if n[0] == "mattes"]
    rest = sum(bool(w["rest_count"].any()) for _, _, w in notes)
    two = sum(bool((w["layer_count"] > 0).sum(0).max() >= 2) for _, _, w in notes)
    selected = sum(bool(info["select"]) and bool(w["select"][0].any()) for _, info, w in notes)
    other = sum(info["window"][2] != SC.SCENES[EDITED]["samples"] for _, info, _ in notes)
    print(f"edit seeds: {len(shares)} edits shown by a frame change {min(shares):.3f}..{max(shares):.3f} of the pixels; {pairs} consecutive matte "
          f"steps under different states or tables, {differing} differ; of {len(notes)} mattes {rest} overflow into rest, {two} hold a pixel of two "
          f"layers, {selected} select an id that is hit, {other} take another sample count than the scene's")
    assert len(shares) >= 20 and min(shares) >= SC.MIN_EDIT_CHANGED
    assert pairs == differing >= 10
    assert rest >= 1 and two >= 1 and selected >= 1 and other >= 1  # (each figure says that a branch of the definition is taken at all)
    assert SC.shows_its_edits(EDITED, frames, events)


def test_the_model_is_right_about_looks():
    """Planes and mattes of an edited look are those of a scene built with the look's fields from the start: the scenario with the
    arrays in place, gridded, cropped, deformed and posed by the helpers of the motion tests, not by the model's Worlds."""
    import copy
    import matte_oracle as MA
    import scenarios
    parts = SC.look_parts(EDITED)
    looks = [("sun_spot", "own", (1, 6)), ("many65", "lambert2", (0, 2)), ("none", "hall", (1, 4)), ("own", "hall", (0, 2)), ("sun", "own", (1, 2))]
    states = [("home", "home"), ("pan", "twist"), ("orbit90", "collapse"), ("shifted", "normals"), ("inside", "scale")]
    for look, (pose, shape) in zip(looks, states):
        sc = getattr(scenarios, EDITED)()
        for k, v in {**parts["lights"][look[0]], **parts["materials"][look[1]]}.items():
            setattr(sc, k, v)
        own = parts["ids"][look[2][0]]
        sc.tri_material = np.where(own < 0, own, own % look[2][1]).astype(np.int32)
        O_ = copy.copy(sc)
        O_.box_min, O_.grid_start, O_.grid_list = O.oracle_scene_grid(O_)
        cropped = MC.crop(O_, *SC.SCENES[EDITED]["size"])
        bent = GC.with_arrays(cropped, *GC.arrays(cropped, shape), lists=False)
        bent.box_min, bent.grid_start, bent.grid_list = O.oracle_scene_grid(bent)
        import camera_cases as CC
        posed = CC.posed(bent, pose)
        want = [np.asarray(p).reshape(posed.height, posed.width) for p in O.oracle_render(posed, threads=16)]
        w = SC.world(EDITED, look)
        assert w.state(pose, shape).material_count == parts["counts"][look[1]] and w.state(pose, shape).light_count == posed.light_count
        for ch, g, x in zip("RGB", w.planes(pose, shape), want):
            assert np.array_equal(g, x), (look, pose, shape, ch)
        assert GC.changed_share(want, SC.world(EDITED).planes(pose, shape)) >= SC.MIN_EDIT_CHANGED, (look, pose, shape)
        s = SC.Session(SC.world(EDITED), (pose, shape), edit=True)
        s.look = look
        s.apply(("mattes", ("material", 2, 8, (4, 1, 3))))
        ids = MA.sample_ids(posed, 4, 1, 3)
        table = MA.material_table(sc.tri_material)
        _, info, got = s.notes[-1]
        ref = MA.mattes(ids, table, info["select"], 8, 3, shape=(posed.height, posed.width))
        for k in ("select", "layer_id", "layer_coverage", "rest"):
            assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (look, k)
        assert (ref["layer_count"] > 0).any()


# ---- the post seeds: the temporal clamp, motion blur and depth of field ------------------------------------------------------------------------
def post_notes():
    """[(scene, seed, part, notes)] of the post seeds' sequences, the model alone."""
    return [(name, seed, part, played(name)[0][seed, part]) for name in SC.SCENES for seed in SC.post_seeds(name)
            for part in range(len(SC.sequences(name, seed)))]


def test_no_shape_changes_the_triangle_count():
    """Why "a reference made for another triangle count" is not among the motion blur's refusals in session_cases.Lite.refuses."""
    for name, spec in SC.SCENES.items():
        base = SC.world(name).base
        for shape in spec["shapes"]:
            _, index, _ = GC.arrays(base, shape)
            assert index is None or np.asarray(index).shape[0] == base.triangle_count, (name, shape)


def test_the_post_seeds_play_the_clamp_and_the_blurs_between_all_other_operations():
    events, per_seed = [], {}
    for name in SC.SCENES:
        for seed in SC.post_seeds(name):
            mine = []
            for q in SC.sequences(name, seed):
                s = SC.lite_of(name, seed, q["start"])
                for step in q["steps"]:
                    s.advance(step)
                mine.append(s.log.events)
            per_seed[name, seed] = SC.post_counts(mine)
            events += mine
    counts = SC.post_counts(events)
    print(f"post seeds: {counts}; per seed {per_seed}")
    assert sorted(per_seed) == [("axis_near_axis_mixed", 118), ("mirror_hall", 36), ("mirror_hall", 118)]
    for k in SC.POST_FACTS:
        assert counts[k] >= 2, f"{k} occurs {counts[k]} times over the post seeds"
    for (name, seed), mine in per_seed.items():
        walk = seed in SC.SCENES[name]["post_walks"]
        assert SC.post_caps(mine, walk, R.tile_count(*SC.SCENES[name]["size"])), (name, seed)
    steps = [(k, a) for name in SC.SCENES for seed in SC.post_seeds(name) for q in SC.sequences(name, seed) for k, a in q["steps"]]
    clamps = [a for k, a in steps if k == "clamp"]
    assert any(a is None for a in clamps) and any(a is not None and a[0] == "refused" for a in clamps)
    assert {a[0] for a in clamps if a is not None and a[0] != "refused"} == set(SC.TCC.MODES), "a mode of the clamp is never set"
    assert any(a is not None and a[0] != "refused" and a[1] == 0.0 for a in clamps), "gamma 0 is never set"
    for kind, table in (("motion_blur", SC.BC.SCENE_PARAMS), ("dof", SC.DC.SCENE_PARAMS)):
        assert {a for k, a in steps if k == kind} == set(range(len(table))), kind


def test_the_post_seeds_clamp_and_blurs_are_not_vacuous():
    """On the oracles alone: the clamp changes the accumulation where a history is live, the blurs gather and change their frames.  Each
    measured share is asserted at half of session_cases.POST_SHARES, which leaves room for another draw."""
    clamped, blurs, dofs = [], [], []
    for name, seed, part, notes in post_notes():
        clamped += [(info, share) for k, info, share in notes if k == "clamped"]
        blurs += [info for k, info, _ in notes if k == "motion_blur"]
        dofs += [info for k, info, _ in notes if k == "dof"]
    live = [share for info, share in clamped if info["live"] and info["cap"] > 1]
    moved = [info for info in blurs if info["mark_differs"]]
    print(f"post seeds: {len(clamped)} accumulation steps under the clamp, {len(live)} with a live history and max_history above 1: the clamped "
          f"oracle's colour differs from the unclamped one's in {np.mean(live):.3f} of the pixels ({min(live):.3f}..{max(live):.3f}), in some pixel "
          f"in {sum(s > 0 for s in live)} of them; {len(blurs)} motion blurs, {len(moved)} with a mark that differs from the state, "
          f"{sum(i['stale'] for i in blurs)} of a stale frame: gather share {np.mean([i['gathered'] for i in blurs]):.3f} over all, "
          f"{np.mean([i['gathered'] for i in moved]):.3f} over the moved ones, {sum(i['changed'] for i in blurs)} change their frame; "
          f"{len(dofs)} depths of field, {sum(i['stale'] for i in dofs)} of a stale frame, {sum(i['window'] != 'default' for i in dofs)} under "
          f"another window: gather share {np.mean([i['gathered'] for i in dofs]):.3f} ({min(i['gathered'] for i in dofs):.3f}.."
          f"{max(i['gathered'] for i in dofs):.3f}), {sum(i['changed'] for i in dofs)} change their frame")
    assert len(live) >= 4 and np.mean(live) >= 0.5 * SC.POST_SHARES["clamped"] > 0
    assert np.mean([i["gathered"] for i in blurs]) >= 0.5 * SC.POST_SHARES["motion_blur_gathered"] > 0
    assert np.mean([i["gathered"] for i in dofs]) >= 0.5 * SC.POST_SHARES["dof_gathered"] > 0
    assert all(i["changed"] for i in dofs), "a depth of field returns its frame"
    assert all(i["changed"] == (i["gathered"] > 0) for i in blurs), "a motion blur that gathers returns its frame, or one that only copies changes it"
    assert all(i["gathered"] > 0 for i in moved), "a motion blur against another state than the mark's gathers nothing"
    off = [share for info, share in clamped if not info["live"]]
    assert all(s == 0.0 for s in off)  # (without a live history the clamp has nothing to pull: the frame itself)


# ---- the sequences played under a layout ----------------------------------------------------------------------------------------------
def test_the_layouts_put_every_operation_between_a_settled_frame_and_a_later_frame():
    """The 58 sequences that tests/test_session_gpu.py plays once more under a layout (session_cases.LAYOUT_SEEDS), on the light model
    alone: how many frames settle (are rendered three times, so that launch plan, placement tables and clean control words are live),
    in which path class, and how often each kind of step stands where it can leave that state stale and have a frame show it."""
    facts = {(name, seed): SC.layout_facts(name, seed) for name, seed in dict.fromkeys((n, s) for _, n, s in SC.LAYOUT_SEEDS)}
    for key, f in facts.items():
        print(f"under a layout, {key}: {f}")
    assert facts == SC.COUNTS_LAYOUT, "the draw or the model changed: measure again"
    assert len(SC.layout_parts()) == 58 and set(SC.LAYOUT_SEEDS) <= {(lay, n, s) for lay in SC.LAYOUTS for n in SC.SCENES for s in SC.seeds_of(n)}
    assert [p[:3] for p in SC.layout_parts()] == [p for _, n, s in SC.LAYOUT_SEEDS for p in SC.all_parts() if p[:2] == (n, s)]
    for name, seed, part, layout in SC.layout_parts():  # a settled frame is one of the default or of a fixed window: every repeat is the same frame
        q = SC.part_of(name, seed, part)
        s = SC.lite_of(name, seed, q["start"])
        for step in q["steps"]:
            s.advance(step)
        for f in s.frames:
            assert not f["settled"] or (f["kind"] in ("default", "fixed") and not f["continuing"] and not f["window"][4]), f
    per_layout = {}
    for layout in SC.LAYOUTS:
        mine = [facts[n, s] for lay, n, s in SC.LAYOUT_SEEDS if lay == layout]
        between = collections.Counter()
        for f in mine:
            between.update(f["between"])
        per_layout[layout] = dict({k: sum(f[k] for f in mine) for k in ("sequences", "steps", "settled", "single", "settled_class", "settled_general", "clones")},
                                  between=dict(between))
        print(f"layout {layout}: {per_layout[layout]}")
        uncovered = tuple(k for k in SC.KINDS_ALL if not between.get(k, 0))
        assert uncovered == SC.LAYOUT_UNCOVERED[layout], f"layout {layout} leaves uncovered: {uncovered}"
        for k in SC.LAYOUT_UNCOVERED[layout]:
            assert k in SC.__doc__.split("Layouts.")[1], f"{k}: not named in session_cases' docstring"
    assert sum(v["sequences"] for v in per_layout.values()) == 58
    # direct: the class's edit circuit and walk alone hold every kind of their alphabet that is not refused, with 20 settled frames in the class
    both = collections.Counter()
    for seed in (21, 110):
        both.update(facts["class_textured_bumped", seed]["between"])
    assert all(both[k] >= 1 for k in SC.KINDS_EDIT), [k for k in SC.KINDS_EDIT if not both[k]]
    assert sum(facts["class_textured_bumped", seed]["settled_class"] for seed in (21, 110)) >= 20
    assert per_layout["direct"]["settled_general"] >= 20  # (and as many that must scatter every ordered round and stay right)
    for layout in ("cut", "groups"):
        for k in ("camera", "shape", "passes", "pipeline", "window"):
            assert per_layout[layout]["between"][k] >= 1, (layout, k)
    assert facts["axis_near_axis_mixed", 3]["between"].get("window", 0) == 0 < facts["axis_near_axis_mixed", 106]["between"]["window"]
    assert per_layout["direct_unsplit"]["settled_class"] >= 4 and per_layout["cut"]["settled_class"] >= 4
    # the four tiles of the groups layout's scene: three groups, and clones of a tile subset among its steps
    assert R.tile_count(*SC.SCENES["axis_near_axis_mixed"]["size"]) == 4
    assert any(k == "clone" and a for s in (3, 106) for q in SC.sequences("axis_near_axis_mixed", s) for k, a in q["steps"])


def test_the_model_gives_what_the_clamp_and_blur_tests_compute_from_their_oracles():
    """Played without a device, the model's expected arrays for the hand-written chains of the three features' own GPU tests are what
    those tests compute directly from their oracles: a relight under the clamp (tests/test_temporal_clamp_gpu.py; here on the scene
    whose looks the model can edit, under a still camera), the camera moves of tests/test_motion_blur_gpu.py, and home / pan / twist of
    tests/test_dof_gpu.py with the depth pass restated by sample_window_cases.window_passes."""
    import motion_blur_oracle as BO
    import dof_oracle as DO
    import temporal_clamp_oracle as CO
    import variance_oracle as VO
    # the relight under the clamp, with and without moments
    w = SC.world(EDITED)
    sc = w.base
    flow = MO.motion(sc, sc)
    looks = [("sun", "own", SC.default_look(EDITED)[2]), ("many65", "own", SC.default_look(EDITED)[2])]
    frames = [np.stack(SC.world(EDITED, look).planes("home", "home"), -1).astype(F32) / F32(65535.0) for look in looks]
    assert not np.array_equal(frames[0], frames[1])
    for clamp in ((3, 1.0), (1, 1.0), (2, 0.5)):
        for kind, empty in (("temporal", TO.empty_history), ("variance", VO.empty_history)):
            s = SC.Session(w, edit=True, post=True)
            s.apply(("clamp", clamp))
            hist, outs = empty(w.height, w.width), []
            for look, frame in zip(looks, frames):
                s.apply(("lights", look[0]))
                s.apply(("frame", None))
                s.apply((kind, (False, 32)))
                want = CO.accumulate(frame, flow["motion"], flow["prev_t"], flow["triangle"], hist, mode=clamp[0], gamma=clamp[1])
                hist = CO.next_history(want, flow["t"], flow["triangle"])
                outs.append(want)
                for k in ("colour", "count"):
                    assert TO.same_bits(s.history[k], want[k]).all(), (clamp, kind, look, k)
                if kind == "variance":
                    assert TO.same_bits(s.moments, want["moments"]).all(), (clamp, look)
            assert s.clamp == clamp and (outs[1]["count"] == 2.0).mean() > 0.1 and (outs[1]["moved"] != 0).any(), "the relight pulled no history in"
    # the camera moves under the motion blur
    w = SC.world("mirror_hall")
    s = SC.Session(w, post=True)
    s.apply(("mark", None))
    for pose, cur, ref, mark, _ in MC.camera_steps(w.base):
        if mark:
            s.apply(("mark", None))
        s.apply(("camera", pose))
        s.apply(("frame", None))
        moved = MO.motion(cur, ref)
        colour = np.stack(w.planes(pose, "home"), -1).astype(F32) / F32(65535.0)
        for variant, params in enumerate(SC.BC.SCENE_PARAMS):
            s.apply(("motion_blur", variant))
            assert BO.same_bits(s.notes[-1][2], BO.blur(colour, moved["motion"], moved["t"], **params)).all(), (pose, params)
    # home / pan / twist under the depth of field
    s = SC.Session(w, post=True)
    s.apply(("passes", R.PASS_DEPTH))
    blurred = 0
    for kind, arg in ((None, None), ("camera", "pan"), ("shape", "twist")):
        if kind:
            s.apply((kind, arg))
        s.apply(("frame", None))
        state = w.state(*s.here())
        depth = WC.window_passes(state, state.sample_count, 0)["depth"]
        colour = np.stack(w.planes(*s.here()), -1).astype(F32) / F32(65535.0)
        focus = float(np.median(depth[np.isfinite(depth) & (depth > 0)]))
        for variant, params in enumerate(SC.DC.SCENE_PARAMS):
            s.apply(("dof", variant))
            _, info, out = s.notes[-1]
            assert info["focus"] == focus and DO.same_bits(out, DO.blur(colour, depth, focus=focus, **params)).all(), (s.here(), params)
            blurred += info["changed"]
    assert blurred == 6 and s.mark is None and s.history is None and s.clamp is None  # (the blurs left the model alone)


# ---- the model against the chains of the motion and temporal tests ---------------------------------------------------------------------------
def same_state(got, want, label, camera=True):
    for k in (("eye", "eye_to_top_left", "left_to_right", "top_to_bottom") if camera else ()) + ("vertex", "tri_index"):
        assert np.asarray(getattr(got, k)).tobytes() == np.asarray(getattr(want, k)).tobytes(), (label, k)
    assert float(got.pixel_size_inv) == float(want.pixel_size_inv), label


def same_flow(got, want, label):
    for k in want:
        assert MO.same_bits(got[k], want[k]).all(), (label, k)


def test_the_model_gives_the_states_and_references_of_the_motion_chains():
    w = SC.world("mirror_hall")
    sc = w.base
    s = SC.Session(w)
    s.apply(("mark", None))
    for (pose, mark), (_, cur, ref, _, _) in zip(MC.CAMERA_SEQUENCE, MC.camera_steps(sc)):
        if mark:
            s.apply(("mark", None))
        s.apply(("camera", pose))
        s.apply(("motion", None))
        same_state(w.state(*s.here()), cur, f"camera/{pose}: current")
        same_state(w.state(*s.mark), ref, f"camera/{pose}: reference")
        same_flow(w.flow(s.here(), s.mark), MO.motion(cur, ref), f"camera/{pose}")
    s = SC.Session(w)
    s.apply(("mark", None))
    for (name, mark), (_, _, cur, ref, _, _) in zip(MC.GEOMETRY_SEQUENCE, MC.geometry_steps(sc)):
        if mark:
            s.apply(("mark", None))
        s.apply(("shape", name))
        s.apply(("motion", None))
        same_state(w.state(*s.here()), cur, f"geometry/{name}: current")
        same_state(w.state(*s.mark), ref, f"geometry/{name}: reference")
        assert np.array_equal(w.state(*s.here()).grid_list, cur.grid_list), name
        same_flow(w.flow(s.here(), s.mark), MO.motion(cur, ref), f"geometry/{name}")
    assert len(s.notes) == len(MC.GEOMETRY_SEQUENCE)


def test_the_model_gives_the_histories_of_the_temporal_camera_chain():
    w = SC.world("mirror_hall")
    chain = TC.camera_chain(w.base)
    flows = TC.chain_flows([(cur, ref) for _, cur, ref in chain])
    s = SC.Session(w)
    hist = TO.empty_history(w.height, w.width)
    for i, ((pose, cur, ref), flow) in enumerate(zip(chain, flows)):
        if i:
            s.apply(("camera", pose))
        s.apply(("frame", None))
        s.apply(("temporal", (False, 32)))
        colour = np.stack(w.planes(pose, "home"), -1).astype(F32) / F32(65535.0)
        want = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist)
        hist = TO.next_history(want, flow["t"], flow["triangle"])
        for k in hist:
            assert TO.same_bits(s.history[k], hist[k]).all(), (pose, k)
        assert s.mark == s.here()
    assert (hist["count"] > 1.0).any()
    s.apply(("reset_temporal", None))
    assert s.history is None
