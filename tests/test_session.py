"""The session sequences without a GPU (tests/session_cases.py; tests/test_session_gpu.py plays them on the device): generation is
deterministic, every circuit holds every ordered pair of kinds exactly once and cutting loses none, camera and shape steps change the
state; on the oracles alone the visited states are not vacuous (hit shares, changed shares), the caps hold (refusals, accepting
temporal steps, a temporal step on an older frame and a motion step with camera and shape both changed in every circuit), and the
model, driven through the chains of motion_cases.py and temporal_cases.py, gives exactly their states, references and histories."""
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
    return [(name, seed) for name, spec in SC.SCENES.items() for seed in spec["circuits"] + spec["wide_circuits"]]


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
        s = SC.Lite(*q["start"], samples=SC.SCENES[name]["samples"])
        for step in q["steps"]:
            s.advance(step)
        end = (s.pose, s.shape)
    alphabet = SC.kinds_of(name, seed)
    K = len(alphabet)
    assert K == (19 if seed in SC.SCENES[name]["wide_circuits"] else 17)
    assert len(kinds) == K * K + 1 and kinds[0] == kinds[-1]
    pairs = collections.Counter(zip(kinds, kinds[1:]))
    assert len(pairs) == K * K and set(pairs.values()) == {1} and set(k for k, _ in pairs) == set(alphabet)
    within = collections.Counter(p for q in parts for p in zip([k for k, _ in q["steps"]], [k for k, _ in q["steps"]][1:]))
    assert within == pairs, "a pair is adjacent in the circuit but in none of its sequences"


def test_camera_and_shape_steps_change_the_state_and_refusals_stay_rare():
    for name, seed, part, q in every_sequence():
        S = SC.SCENES[name]["samples"]
        s, refused = SC.Lite(*q["start"], samples=S), 0
        for kind, arg in q["steps"]:
            assert kind in SC.kinds_of(name, seed)
            if kind == "window" and arg is not None:
                win = arg[1] if s.refuses((kind, arg)) else arg
                rc = R.lib().rtHipSampleWindowCheck(S, C.byref(R.SampleWindow(*win)))
                if s.refuses((kind, arg)):
                    assert rc == -1 and arg[2] in R.last_error(), (name, seed, part, arg, R.last_error())
                else:
                    assert rc == 0 and win[0] in [S * n for n in SC.WINDOW_SIZES], (name, seed, part, arg, R.last_error())
                    assert not (win[3] and win[1] > 0), "a window that continues is drawn at f = 0 only: it never starts on an undefined buffer"
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
        for seed in spec["walks"] + spec["wide_walks"]:
            parts = SC.sequences(name, seed)
            assert sum(len(q["steps"]) for q in parts) == SC.WALK + len(parts) - 1  # (a cut walk repeats the kind it was cut at)
            assert all(len(q["steps"]) <= spec.get("walk_cut", SC.WALK) for q in parts) and ("walk_cut" in spec or len(parts) == 1)
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
            s = SC.Session(w, q["start"])
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
        assert hits[-1] >= MC.MIN_HIT, f"{name}/{st}: only {hits[-1]:.3f} of the centre rays hit"
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
    opaque-diffuse class only, and both scenes are of the general class."""
    for name in SC.SCENES:
        assert R.path_class(SC.world(name).base) == R.PATH_CLASS_GENERAL, name


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
