"""Resident scenes under sequences of operations: a model of the scene's state, the operations with their effect on the model and their
check, and the seeded sequences (tests/test_session.py shows on the oracles alone that they are not vacuous and that the model is right,
tests/test_session_gpu.py plays them on the device, tests/session_replay.py plays one by hand).

State.  The model (Session) holds the pose (camera_cases.POSES + "shifted") and the shape (geometry_cases.SEQUENCE, deformations of the
BASE scene), the pass mask, the pipeline, the last rendered frame (its planes and the pose, shape and mask it was rendered under), the
motion reference (pose and shape at the mark, or none), the temporal history (temporal_oracle's arrays; None = reset or never made),
whether an update has succeeded (the scene retains an index array from then on) and the pose ResidentScene.scene describes (the one of
creation or of the last update: a camera move does not touch that copy).  The 5 x 7 Scenes of a base scene (fewer where a scene's
shapes are narrowed) are cached in a World with the oracle's grid, camera lists, planes, centre-ray walks and flows.

Checks.  Frames equal oracle_render as integers; lists and device arrays equal the oracle's after every move and update; motion equals
motion_oracle against the model's mark; temporal equals temporal_oracle.accumulate over the model's LAST RENDERED planes, the flow of the
CURRENT state against the model's mark, and the model's history; refusals return their code and text and change nothing, which every
later check proves.  Passes, denoise, AO and the bake are compared with a twin: a ResidentScene created fresh from the model's Scene
(made once per visited state and closed at once, its products cached for the module); a fresh scene's products are pinned to their
oracles by the feature tests.  The denoiser is also compared with denoise_oracle on the read-backs, and on the small scene AO and the
bake with ao_oracle and bake_oracle, so that twin and subject cannot be wrong alike.

What the header leaves open is not checked: read_passes, denoise and temporal(denoise=) read buffers that a frame fills under the mask
in effect, so where no frame has been rendered yet, or the last one was rendered under another mask, the operation renders one first
(checked like any frame).  So "A directly followed by B" holds for the kinds of a circuit, while on the device a frame stands between
passes -> read_passes, passes -> denoise, passes -> temporal(denoise=) and between a fresh scene and any of the three.  A stale pose
or shape is defined -- the products are the old frame's -- and is left stale on purpose.

Sequences.  A circuit is an Eulerian circuit of the complete directed graph on the K kinds, loops included: K * K + 1 steps in which
every ordered pair of kinds is adjacent exactly once.  It is cut into sequences of at most CUT steps (fewer on the larger scene, see
SCENES).  A cut is placed as late as the refusal cap allows: a sequence is the longest run whose refusals are at most a fifth of its
steps and after which the rest of the circuit can still be cut that way.  Each sequence starts from a fresh scene, at the pose and
shape the one before ended in, and its first step repeats the previous one's last kind, so no pair is lost at a cut.
Arguments are drawn against a light copy of the state so that camera and shape steps always change something and refusals stay rare;
a draw that misses one of the caps below is drawn again (attempt 0, 1, ...): generation is a pure function of (scene, seed)."""
import numpy as np

import ao_oracle
import bake_oracle
import camera_cases as CC
import denoise_oracle as D
import geometry_cases as GC
import motion_cases as MC
import motion_oracle as MO
import oracle_lib as O
import prep_oracle as P
import query_cases as Q
import temporal_oracle as TO
from geometry_checks import assert_device_arrays, prep_of, update_to
from opencl_render_amd import raytrace as R

F32 = np.float32
NONE = 0xFFFFFFFF
KINDS = ("frame", "camera", "shape", "passes", "pipeline", "read_passes", "denoise", "ao", "bake", "intersect", "mark", "motion", "temporal",
         "reset_temporal", "refused_update", "refused_camera", "clone")
K = len(KINDS)
POSES = CC.POSES + ("shifted",)
NEAR = ("home", "pan", "shifted")
SURFACE = R.PASS_NORMAL | R.PASS_ALBEDO
MASKS = (SURFACE, 31, SURFACE | R.PASS_ALPHA, SURFACE, 30, 31, 0, R.PASS_NORMAL, 7)  # mostly with both surface passes: the denoiser runs
DENOISE_VARIANTS = ({}, dict(iterations=3, colour_inv_sigma2=0.5))
TEMPORAL_DENOISE = dict(iterations=2, colour_inv_sigma2=0.5)
MAX_HISTORY = (1, 4, 32)
UPDATE_REFUSALS = ("index", "negative", "smaller_v", "host_pointer", "list_limit")
CUT, WALK = 40, 60
MAX_REFUSED = 0.2  # of any sequence's steps
MIN_WARM = 0.35  # of a seed's temporal steps follow another one of their sequence, with no reset and no update between
# Scenes, with their circuit and walk seeds and the shapes drawn for them.  axis_near_axis_mixed loses "translate": from orbit90 the
# translated mesh is hidden, and the oracle's planes of translate, reindex and home are the same there.
SCENES = {"mirror_hall": dict(size=(24, 16), circuits=(1, 2), walks=(101, 102), shapes=GC.SEQUENCE, cut=40),
          "axis_near_axis_mixed": dict(size=(136, 132), circuits=(3,), walks=(), shapes=tuple(n for n in GC.SEQUENCE if n != "translate"), cut=25,
                                       shape_steps=2)}
# Measured on the oracle by tests/test_session.py, which prints them, over the visited states (hit share of the centre rays; share of the
# oracle's pixels that differ between the two states of a camera or shape step, home <-> reindex excepted as in geometry_cases.py):
# mirror_hall 31 states visited, hit share 0.596..0.979, changed share 0.602..1.000 over 70
# distinct moves; axis_near_axis_mixed 17 states, hit share 0.746..1.000, changed share 0.195..1.000 over 32 moves; 21 of 62 temporal steps
# accept history in at least 0.2 of the pixels.  COUNTS is asserted there, so that a change of the draw cannot leave these figures behind.
COUNTS = dict(sequences=34, steps=1019)
SMALL = "mirror_hall"  # AO and the bake are also compared with their numpy oracles here
# Reduced sequences of mismatches found by the circuits: name -> (scene, (start pose, start shape), steps).  None so far.
REGRESSIONS = {}


def flags(mask):
    return dict(alpha=bool(mask & R.PASS_ALPHA), depth=bool(mask & R.PASS_DEPTH), triangle=bool(mask & R.PASS_TRIANGLE),
                normal=bool(mask & R.PASS_NORMAL), albedo=bool(mask & R.PASS_ALBEDO))


# ---- the oracle's view of a base scene's 5 x 7 states -------------------------------------------------------------------------------
class World:
    def __init__(self, name):
        self.name, self.size = name, SCENES[name]["size"]
        self.base = MC.base_scene(name, self.size)
        self.width, self.height = self.base.width, self.base.height
        self._shape, self._state, self._planes, self._trace, self._flow, self._prep = {}, {}, {}, {}, {}, {}

    def shape_scene(self, shape):
        if shape not in self._shape:
            sc = GC.with_arrays(self.base, *GC.arrays(self.base, shape), lists=False)
            sc.box_min, sc.grid_start, sc.grid_list = O.oracle_scene_grid(sc)
            self._shape[shape] = sc
        return self._shape[shape]

    def prep(self, shape):
        """prep_oracle's records and dense view of the shape (seconds on the larger scene's grid, and a circuit updates to the same
        few shapes many times)."""
        if shape not in self._prep:
            self._prep[shape] = prep_of(self.shape_scene(shape))
        return self._prep[shape]

    def warm(self, states):
        """Everything the checks read of the given (pose, shape) states, made now: a test module's fixture calls this once, so that a
        sequence's time is the device's and the comparisons'."""
        for pose, shape in states:
            self.planes(pose, shape)
            self.trace(pose, shape)
            self.prep(shape)

    def state(self, pose, shape):
        """The Scene of (pose, shape) with the oracle's grid and camera lists."""
        if (pose, shape) not in self._state:
            self._state[pose, shape] = CC.posed(self.shape_scene(shape), pose)
        return self._state[pose, shape]

    def planes(self, pose, shape):
        """oracle_render of the state: three [H, W] u16 planes."""
        if (pose, shape) not in self._planes:
            sc = self.state(pose, shape)
            self._planes[pose, shape] = [np.asarray(p).reshape(sc.height, sc.width).copy() for p in O.oracle_render(sc, threads=16)]
        return self._planes[pose, shape]

    def trace(self, pose, shape):
        if (pose, shape) not in self._trace:
            self._trace[pose, shape] = MO.trace(self.state(pose, shape))
        return self._trace[pose, shape]

    def flow(self, cur, ref):
        """motion_oracle.motion of state `cur` against the reference state `ref` ((pose, shape) each)."""
        if (cur, ref) not in self._flow:
            self._flow[cur, ref] = MO.project(self.state(*cur), self.state(*ref), self.trace(*cur))
        return self._flow[cur, ref]


_worlds = {}


def world(name):
    if name not in _worlds:
        _worlds[name] = World(name)
    return _worlds[name]


# ---- twins ---------------------------------------------------------------------------------------------------------------------------
_twin, _twin_ao, _twin_bake, _oracle_ao, _oracle_bake = {}, {}, {}, {}, {}


def twin(w, pose, shape, mask):
    """What a scene created fresh from the state returns under `mask`: {"passes", "denoise" (one per variant, with both surface
    passes)}; its AO image and bake go to caches of their own (they do not depend on the mask, the bake not on the pose either)."""
    key = (w.name, pose, shape, mask)
    if key not in _twin:
        t = R.ResidentScene(w.state(pose, shape), 0)
        try:
            out = {}
            if mask:
                t.set_passes(**flags(mask))
            t.render()
            out["passes"] = t.readback_passes()
            if mask & SURFACE == SURFACE:
                out["denoise"] = [t.denoise(**v) for v in DENOISE_VARIANTS]
            if (w.name, pose, shape) not in _twin_ao:
                _twin_ao[w.name, pose, shape] = t.ambient_occlusion(rays=4)
            if (w.name, shape) not in _twin_bake:
                _twin_bake[w.name, shape] = t.bake_ambient_occlusion(16, 16, rays=4, dilate=2)
            _twin[key] = out
        finally:
            t.close()
    return _twin[key]


def twin_ao(w, pose, shape):
    if (w.name, pose, shape) not in _twin_ao:
        twin(w, pose, shape, 0)
    return _twin_ao[w.name, pose, shape]


def twin_bake(w, shape):
    if (w.name, shape) not in _twin_bake:
        twin(w, "home", shape, 0)
    return _twin_bake[w.name, shape]


def differs(got, want, what):
    """Raises with the array's name and the number of differing values (floats as bits, a NaN on both sides equal)."""
    g, x = np.asarray(got), np.asarray(want)
    assert g.shape == x.shape and g.dtype == x.dtype, f"{what}: got {g.dtype} {g.shape}, want {x.dtype} {x.shape}"
    same = TO.same_bits(g, x) if g.dtype == F32 else g == x
    bad = int(same.size - np.count_nonzero(same))
    assert bad == 0, f"{what} differs in {bad} of {x.size} values"


def refusal(call, text, what):
    """call() must raise RuntimeError with `text` in the library's last error."""
    try:
        call()
    except RuntimeError:
        assert text in R.last_error(), f"{what}: refused with {R.last_error()!r}, expected {text!r}"
        return
    raise AssertionError(f"{what}: the call succeeded, expected a refusal ({text!r})")


# ---- the light state the arguments are drawn against, and every kind's expected refusal ----------------------------------------------------
class Lite:
    def __init__(self, pose="home", shape="home"):
        self.pose, self.shape, self.mask, self.pipeline = pose, shape, 0, R.PIPELINE_WAVEFRONT
        self.frame = self.mark = None  # (pose, shape, mask) / (pose, shape)
        self.updated = False

    def refuses(self, step):
        kind, arg = step
        if kind == "passes":
            return self.pipeline == R.PIPELINE_MEGAKERNEL and arg != 0
        if kind == "pipeline":
            return arg == R.PIPELINE_MEGAKERNEL and self.mask != 0
        if kind == "denoise":
            return self.mask & SURFACE != SURFACE
        if kind == "motion":
            return self.mark is None
        if kind == "temporal":
            return arg[0] and self.mask & SURFACE != SURFACE
        if kind == "clone":
            return bool(arg)  # the subset's temporal() is refused
        return kind in ("refused_update", "refused_camera")

    def renders(self, uses_passes):
        return self.frame is None or (uses_passes and self.frame[2] != self.mask)

    def advance(self, step):
        """The step's effect on (pose, shape, mask, pipeline, frame, mark, updated); a refused step has none."""
        kind, arg = step
        if self.refuses(step) and kind != "clone":
            return
        if kind == "camera":
            self.pose = arg
        elif kind == "shape":
            self.shape, self.updated = arg, True
        elif kind == "passes":
            self.mask = arg
        elif kind == "pipeline":
            self.pipeline = arg
        elif kind == "mark":
            self.mark = (self.pose, self.shape)
        if kind == "frame" or (kind in ("read_passes", "denoise") and self.renders(True)) or (kind == "temporal" and self.renders(arg[0])):
            self.frame = (self.pose, self.shape, self.mask)
        if kind == "temporal":
            self.mark = (self.pose, self.shape)


def draw(rng, kind, s, may_refuse, tiles, shapes, seen=()):
    """The argument of a step of `kind` in light state `s`; may_refuse: the sequence can still afford a refusal."""
    pick = lambda seq: seq[int(rng.integers(len(seq)))]  # noqa: E731
    dare = may_refuse and rng.random() < 0.3
    if kind == "camera":  # a pose the circuit has not seen yet goes first, so that every circuit visits all five; after that the draw
        new = [p for p in POSES if p not in seen]  # stays among home, pan and shifted, which lie close together, so that history is accepted
        if new:
            return pick(new)
        near = [p for p in NEAR if p != s.pose]
        return pick(near)
    if kind == "shape":
        return pick([n for n in shapes if n != s.shape])
    if kind == "passes":
        if s.pipeline == R.PIPELINE_MEGAKERNEL:
            return pick([m for m in MASKS if m]) if dare else 0
        return pick(MASKS)
    if kind == "pipeline":
        if s.mask:
            return R.PIPELINE_MEGAKERNEL if dare else R.PIPELINE_WAVEFRONT
        if s.pipeline == R.PIPELINE_MEGAKERNEL:
            return R.PIPELINE_WAVEFRONT if rng.random() < 0.8 else R.PIPELINE_MEGAKERNEL
        return R.PIPELINE_MEGAKERNEL if rng.random() < 0.35 else R.PIPELINE_WAVEFRONT
    if kind == "denoise":
        return int(rng.integers(len(DENOISE_VARIANTS)))
    if kind == "intersect":
        return int(rng.integers(1 << 20))
    if kind == "temporal":
        on = rng.random() < 0.5 if s.mask & SURFACE == SURFACE else dare
        return (bool(on), int(pick(MAX_HISTORY)))
    if kind == "refused_update":
        return (pick(UPDATE_REFUSALS), pick([n for n in shapes if n != s.shape]))
    if kind == "refused_camera":
        return pick([p for p in POSES if p != s.pose])
    if kind == "clone":
        return bool(tiles > 1 and dare)
    return None


def eulerian(rng):
    """K * K + 1 kind indices: a walk that uses every ordered pair of kinds, loops included, exactly once (Hierholzer, the edges of every
    node in a seeded order)."""
    out = [[int(v) for v in rng.permutation(K)] for _ in range(K)]
    stack, path = [int(rng.integers(K))], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def _piece(rng, kinds, start, tiles, shapes, seen):
    """Steps for `kinds` from a fresh scene at `start`, and what the caps ask about them: (steps, refusals after each step, temporal
    steps on an older frame, motion steps with camera and shape both changed, each as the index of the step)."""
    s, steps, refused, stale, mixed = Lite(*start), [], [], [], []
    seen, hist, temporal, warm = set(seen), False, [], []
    for i, k in enumerate(kinds):
        kind = KINDS[k]
        step = (kind, draw(rng, kind, s, (sum(refused[-1:]) + 1) <= MAX_REFUSED * (i + 1), tiles, shapes, seen))
        refused.append((refused[-1] if refused else 0) + bool(s.refuses(step)))
        if kind == "temporal" and not s.refuses(step) and not s.renders(step[1][0]) and s.frame[:2] != (s.pose, s.shape):
            stale.append(i)
        if kind == "motion" and s.mark is not None and s.mark[0] != s.pose and s.mark[1] != s.shape:
            mixed.append(i)
        if kind == "temporal" and not s.refuses(step):  # with a history, and reprojected from the same shape: likely to accept some
            temporal.append(i)
            if hist and s.mark[1] == s.shape:
                warm.append(i)
            hist = True
        if kind == "reset_temporal":
            hist = False
        s.advance(step)
        steps.append(step)
        seen |= {s.pose, s.shape}
    return steps, refused, stale, mixed, temporal, warm


def _attempt(name, seed, attempt):
    """One draw of the seed's sequences, or None where it misses a cap.  A circuit is cut where the refusal cap allows: a piece is the
    longest run of at most the scene's cut whose refusals are at most MAX_REFUSED of its steps, drawn with a generator of its own, and
    the next piece starts with its last kind."""
    spec = SCENES[name]
    key = [sorted(SCENES).index(name), seed, attempt]
    tiles = R.tile_count(*spec["size"])
    walk = seed in spec["walks"]
    kinds = [int(v) for v in np.random.default_rng(key).integers(K, size=WALK)] if walk else eulerian(np.random.default_rng(key))
    limit = WALK if walk else spec["cut"]
    budget = [400]  # pieces tried: a draw that needs more is given up

    def rest(at, start, seen):
        """The pieces from step `at` on, or None: the longest piece that fits first, a shorter one where the rest cannot be cut."""
        if at >= len(kinds) - 1:
            return []
        budget[0] -= 1
        if budget[0] < 0:
            return None
        piece = kinds[at:at + limit]
        steps, refused, st, mx, tp, wm = _piece(np.random.default_rng(key + [at]), piece, start, tiles, spec["shapes"], seen)
        for n in range(len(piece), 1, -1):
            if refused[n - 1] > MAX_REFUSED * n or (walk and n < len(piece)):
                continue
            if sum(k == "shape" for k, _ in steps[:n]) > spec.get("shape_steps", n):
                continue  # (an update's check of the device arrays takes over a second on the larger scene's 12.6 million pairs)
            s, now = Lite(*start), set(seen)
            for step in steps[:n]:
                s.advance(step)
                now |= {s.pose, s.shape}
            tail = rest(at + n - 1, (s.pose, s.shape), now)
            if tail is not None:
                return [dict(start=start, steps=steps[:n], stale=sum(i < n for i in st), mixed=sum(i < n for i in mx), seen=now,
                             temporal=sum(i < n for i in tp), warm=sum(i < n for i in wm))] + tail
        return None

    out = rest(0, ("home", "home"), {"home"})
    if out is None:
        return None
    stale, mixed, seen = sum(q.pop("stale") for q in out), sum(q.pop("mixed") for q in out), set().union(*(q.pop("seen") for q in out))
    if sum(q.pop("warm") for q in out) < MIN_WARM * sum(q.pop("temporal") for q in out):
        return None  # (too few temporal steps with a history to reproject: the accepting share could not reach a third)
    if not walk and not (stale and mixed and seen >= set(POSES) | set(spec["shapes"])):
        return None  # (the camera draw favours the near poses: a circuit still visits every pose and every shape)
    return out


_sequences = {}


def sequences(name, seed):
    """[{"start": (pose, shape), "steps": [(kind, argument)]}] of a circuit or walk seed of scene `name`."""
    if (name, seed) not in _sequences:
        for attempt in range(2000):
            out = _attempt(name, seed, attempt)
            if out is not None:
                break
        else:
            raise RuntimeError(f"{name} seed {seed}: no draw met the caps")
        _sequences[name, seed] = out
    return _sequences[name, seed]


def all_parts():
    """(scene, seed, part) of every sequence; regressions are (scene, name, 0)."""
    out = [(name, seed, part) for name, spec in SCENES.items() for seed in spec["circuits"] + spec["walks"]
           for part in range(len(sequences(name, seed)))]
    return out + [(scene, key, 0) for key, (scene, _, _) in REGRESSIONS.items()]


def visited(name):
    """The (pose, shape) states the scene's sequences pass through, in order of first visit."""
    out = []
    for n, seed, part in all_parts():
        if n == name:
            q = part_of(n, seed, part)
            s = Lite(*q["start"])
            out.append((s.pose, s.shape))
            for step in q["steps"]:
                s.advance(step)
                out.append((s.pose, s.shape))
    return list(dict.fromkeys(out))


def part_of(name, seed, part):
    if seed in REGRESSIONS:
        scene, start, steps = REGRESSIONS[seed]
        return dict(start=start, steps=list(steps))
    return sequences(name, seed)[part]


# ---- the model, and the device beside it ---------------------------------------------------------------------------------------------
class Session(Lite):
    """The model of one resident scene.  With rs (a ResidentScene created from world.state(*start)) every step is also made on the device
    and checked; without, the model advances alone and notes what tests/test_session.py asserts on (self.notes)."""

    def __init__(self, w, start=("home", "home"), rs=None):
        super().__init__(*start)
        self.w, self.rs = w, rs
        self.described_pose = start[0]
        self.planes = self.history = None
        self.notes = []

    def here(self):
        return (self.pose, self.shape)

    def apply(self, step):
        kind, arg = step
        getattr(self, "do_" + kind)(arg) if arg is not None else getattr(self, "do_" + kind)()
        self.advance(step)

    # -- frames
    def do_frame(self):
        want = self.w.planes(*self.here())
        if self.rs:
            self.rs.render()
            sc = self.w.base
            for ch, g, x in zip("RGB", self.rs.readback(), want):
                differs(np.asarray(g).reshape(sc.height, sc.width), x, f"plane {ch} of the frame at {self.here()}")
        self.planes = want

    def need_frame(self, uses_passes):
        if self.renders(uses_passes):
            self.do_frame()
            self.frame = (self.pose, self.shape, self.mask)

    # -- state changes
    def do_camera(self, pose):
        sc = self.w.state(pose, self.shape)
        if self.rs:
            self.rs.set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
            CC.assert_lists_equal(self.rs, sc, f"lists after the move to {pose}")

    def do_shape(self, name):
        want = self.w.state(self.pose, name)
        if self.rs:
            update_to(self.rs, want)
            CC.assert_lists_equal(self.rs, want, f"lists after the update to {name}")
            assert_device_arrays(self.rs, want, f"device arrays after the update to {name}", self.w.prep(name))
        self.described_pose = self.pose

    def do_passes(self, mask):
        if not self.rs:
            return
        if self.refuses(("passes", mask)):
            refusal(lambda: self.rs.set_passes(**flags(mask)), "wavefront pipeline", "passes on the megakernel")
        else:
            self.rs.set_passes(**flags(mask))

    def do_pipeline(self, p):
        if not self.rs:
            return
        if self.refuses(("pipeline", p)):
            refusal(lambda: self.rs.set_pipeline(p), "render passes are on", "the megakernel while passes are on")
        else:
            self.rs.set_pipeline(p)

    # -- products of (pose, shape, mask)
    def do_read_passes(self):
        self.need_frame(True)
        if self.rs:
            got, want = self.rs.readback_passes(), twin(self.w, *self.frame)["passes"]
            assert sorted(got) == sorted(want), f"passes {sorted(got)}, the twin's {sorted(want)}"
            for k in want:
                differs(got[k], want[k], f"pass {k} of the frame at {self.frame}")

    def do_denoise(self, variant):
        params = DENOISE_VARIANTS[variant]
        if self.refuses(("denoise", variant)):
            if self.rs:
                refusal(lambda: self.rs.denoise(**params), "normal and the albedo pass", "denoise without both surface passes")
            return
        self.need_frame(True)
        if self.rs:
            got, want = self.rs.denoise(**params), twin(self.w, *self.frame)["denoise"][variant]
            differs(got["colour"], want["colour"], "denoised colour (against the twin)")
            for ch, g, x in zip("RGB", got["planes"], want["planes"]):
                differs(g, x, f"denoised plane {ch} (against the twin)")
            sc = self.w.base
            planes = [np.asarray(p).reshape(sc.height, sc.width) for p in self.rs.readback()]
            surf = self.rs.readback_passes()
            exp = D.denoise(*D.inputs(planes, surf["normal"], surf["albedo"]), **dict(R.DENOISE_DEFAULTS, **params))
            differs(got["colour"], exp, "denoised colour (against the oracle on the read-backs)")
            for ch, g, x in zip("RGB", got["planes"], D.quantise(exp)):
                differs(g, x, f"denoised plane {ch} (against the oracle on the read-backs)")

    def do_ao(self):
        if self.rs:
            got = self.rs.ambient_occlusion(rays=4)
            differs(got, twin_ao(self.w, *self.here()), "AO image (against the twin)")
            if self.w.name == SMALL:
                key = (self.w.name,) + self.here()
                if key not in _oracle_ao:
                    _oracle_ao[key] = ao_oracle.ambient_occlusion(self.w.state(*self.here()), rays=4)
                differs(got, _oracle_ao[key], "AO image (against the oracle)")

    def do_bake(self):
        if self.rs:
            got, want = self.rs.bake_ambient_occlusion(16, 16, rays=4, dilate=2), twin_bake(self.w, self.shape)
            for k in ("ao", "triangle"):
                differs(got[k], want[k], f"bake {k} (against the twin)")
            if self.w.name == SMALL:
                key = (self.w.name, self.shape)
                if key not in _oracle_bake:
                    _oracle_bake[key] = bake_oracle.bake(self.w.state("home", self.shape), 16, 16, rays=4, dilate_passes=2)
                for k in ("ao", "triangle"):
                    differs(got[k], _oracle_bake[key][k], f"bake {k} (against the oracle)")

    def do_intersect(self, seed):
        if self.rs:
            rng = np.random.default_rng(seed)
            o = (rng.normal(size=(256, 3)) * 0.5 + CC.CENTRE).astype(F32)
            d = rng.normal(size=(256, 3)).astype(F32)
            rays = Q._set(o, d, 0.0, np.inf, NONE)
            got = self.rs.intersect(rays["o"], rays["d"], rays["tmin"], rays["tmax"], rays["excluded"])
            bad = Q.mismatches({k: got[k] for k in ("triangle", "t", "ab", "ac")}, Q.oracle_answers(self.w.state(*self.here()), rays))
            assert bad.size == 0, f"ray query answers differ in {bad.size} of 256 rays"

    # -- motion and temporal accumulation
    def same_mark(self, what):
        cam, sc = self.rs.motion_reference_camera(), self.w.state(*self.here())
        for k in ("eye", "eye_to_top_left", "left_to_right", "top_to_bottom"):
            differs(cam[k][:3], np.asarray(getattr(sc, k), F32)[:3], f"{what}: the reference camera's {k}")

    def do_mark(self):
        if self.rs:
            self.rs.mark_motion()
            self.same_mark("mark")

    def do_motion(self):
        if self.mark is None:  # the header: refused with "no motion reference"
            if self.rs:
                refusal(self.rs.motion, "no motion reference", "motion without a mark")
            return
        want = self.w.flow(self.here(), self.mark)
        self.notes.append(("motion", self.mark[0] != self.pose and self.mark[1] != self.shape, MC.shares(want)[0]))
        if self.rs:
            got = self.rs.motion()
            for k in ("motion", "t", "prev_t", "triangle"):
                differs(got[k], want[k], f"motion output {k} at {self.here()} against the mark at {self.mark}")

    def do_temporal(self, arg):
        on, cap = arg
        if self.refuses(("temporal", arg)):
            if self.rs:
                refusal(lambda: self.rs.temporal(denoise=TEMPORAL_DENOISE, max_history=float(cap)), "normal and the albedo pass",
                        "temporal(denoise=) without both surface passes")
            return
        self.need_frame(on)
        flow = self.w.flow(self.here(), self.mark or self.here())  # no mark yet: the call marks the current state first
        colour = np.stack(self.planes, -1).astype(F32) / F32(65535.0)
        hist = self.history if self.history is not None else TO.empty_history(self.w.height, self.w.width)
        acc = TO.accumulate(colour, flow["motion"], flow["prev_t"], flow["triangle"], hist, max_history=float(cap), with_taps=True)
        self.notes.append(("temporal", self.frame[:2] != self.here(), float(acc["used"].mean())))
        if self.rs:
            shown = acc["colour"]
            if on:
                surf = twin(self.w, *self.frame)["passes"]
                shown = D.denoise(acc["colour"], surf["normal"], surf["albedo"], **dict(R.DENOISE_DEFAULTS, **TEMPORAL_DENOISE))
            got = self.rs.temporal(denoise=TEMPORAL_DENOISE if on else None, max_history=float(cap))
            differs(got["count"], acc["count"], "temporal count")
            differs(got["colour"], shown, "temporal colour")
            for ch, g, x in zip("RGB", got["planes"], D.quantise(shown)):
                differs(g, x, f"temporal plane {ch}")
            self.same_mark("temporal (the call owns the mark)")
        self.history = TO.next_history(dict(colour=acc["colour"], count=acc["count"]), flow["t"], flow["triangle"])

    def do_reset_temporal(self):
        if self.rs:
            self.rs.reset_temporal()
        self.history = None

    # -- refusals: one illegal argument each; nothing changes, which every later check proves
    def do_refused_update(self, arg):
        variant, target = arg
        cur, want = self.w.state(*self.here()), self.w.state(self.pose, target)
        if not self.rs:
            assert len(want.grid_list) > 1
            return
        rs, T, V = self.rs, want.triangle_count, want.vertex_count
        if variant == "index":
            bad = want.tri_index.copy()
            bad[T // 2, 1] = V
            rc, code, text = rs.try_set_vertices(want.vertex, bad), -5, P.rejection_text(P.ERR_TRI_INDEX)
        elif variant == "negative":
            bad = want.tri_index.copy()
            bad[0, 0] = -1
            rc, code, text = rs.try_set_vertices(want.vertex, bad), -5, P.rejection_text(P.ERR_TRI_INDEX)
        elif variant == "smaller_v":  # the retained index array against half the vertices; nothing retained before the first update
            rc = rs.try_set_vertices(cur.vertex[: cur.vertex_count // 2])
            code, text = (-5, P.rejection_text(P.ERR_TRI_INDEX)) if self.updated else (-1, "retained")
        elif variant == "host_pointer":
            rc = int(R.lib().rtHipSceneSetGeometry(rs.handle, R.GeometryUpdate(V, R._ptr(want.vertex), None, None, 1)))
            code, text = -1, "not device memory" if self.updated else "retained"
        else:
            R.tune("build_list_limit", len(want.grid_list) - 1)
            try:
                rc, code, text = rs.try_set_vertices(want.vertex, want.tri_index), -3, "limit"
            finally:
                R.tune("build_list_limit", 0xFFFFFFFF)
        assert rc == code and text in R.last_error(), f"refused update ({variant}): returned {rc} with {R.last_error()!r}, expected {code} with {text!r}"

    def do_refused_camera(self, pose):
        sc = self.w.state(pose, self.shape)
        total = int((sc.cam_end.astype(np.int64) - sc.cam_start).sum())
        assert total > 0
        if self.rs:
            R.tune("build_list_limit", total - 1)
            try:
                rc = self.rs.try_set_camera(sc.eye, sc.eye_to_top_left, sc.left_to_right, sc.top_to_bottom, sc.pixel_size_inv)
            finally:
                R.tune("build_list_limit", 0xFFFFFFFF)
            assert rc == -3 and "limit" in R.last_error(), f"refused move: returned {rc} with {R.last_error()!r}, expected -3"

    def do_clone(self, subset):
        """An instance made like the scene from the scene's own description (the pose of creation or of the last update)."""
        if not self.rs:
            return
        sc = self.w.base
        tiles = np.arange(R.tile_count(sc.width, sc.height), dtype=np.uint32)[1:] if subset else None
        # (the scene's own description rebuilds its lists with the host builders when read, which takes seconds on the larger scene's
        # rooms: there the clone is described by the model's Scene of the same pose and shape)
        desc = self.rs.scene if self.w.name == SMALL else self.w.state(self.described_pose, self.shape)
        c = R.ResidentScene(desc, 0, tiles, like=self.rs)
        try:
            c.render()
            got = [np.asarray(p).reshape(sc.height, sc.width) for p in c.readback()]
            mine = np.ones((sc.height, sc.width), bool)
            if subset:
                mine[:R.TILE, :R.TILE] = False  # tile 0 is not the clone's
                refusal(c.temporal, "every tile of the image", "temporal on a tile subset")
            for ch, g, x in zip("RGB", got, self.w.planes(self.described_pose, self.shape)):
                differs(g, np.where(mine, x, 0).astype(np.uint16), f"plane {ch} of the clone's frame")
        finally:
            c.close()


def describe(steps):
    return "; ".join(f"{i}: {k}" + ("" if a is None else f"({a})") for i, (k, a) in enumerate(steps))


def play(name, seed, part, last=None, report=None):
    """Plays one sequence on the device and stops at the first mismatch: one pass, nothing is tried again.  The scene is always closed
    (twins and clones close themselves).  report(step number, step, verdict) is called after every step."""
    seq = part_of(name, seed, part)
    steps = seq["steps"] if last is None else seq["steps"][:last + 1]
    w = world(name)
    rs = R.ResidentScene(w.state(*seq["start"]), 0)
    try:
        s = Session(w, seq["start"], rs)
        for i, step in enumerate(steps):
            try:
                s.apply(step)
            except (AssertionError, RuntimeError) as e:
                if report:
                    report(i, step, f"MISMATCH: {e}")
                raise AssertionError(f"{name} seed {seed} part {part}, step {i} {step}: {e}\nstarted at {seq['start']}; steps so far: "
                                     f"{describe(steps[:i + 1])}") from e
            if report:
                report(i, step, "ok")
    finally:
        rs.close()
    return len(steps)
