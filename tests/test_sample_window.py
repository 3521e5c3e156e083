"""Sample windows without a GPU: the host-only check of a window (every refusal with its own text, the legal edges), the ABI's shape,
and the premises of the divisor test of tests/test_sample_window_gpu.py, from the committed goldens."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import sample_window_cases as WC
from conftest import ROOT, golden_names
from opencl_render_amd import raytrace as R

U32_MAX = WC.U32_MAX


def check(samples, *window):
    """(return code, last-error text) of rtHipSampleWindowCheck(samples, {total, first, divisor, accumulate, advance})."""
    w = R.SampleWindow(*window)
    rc = R.lib().rtHipSampleWindowCheck(samples, C.byref(w))
    return rc, R.last_error()


def test_header_python_and_library_agree(hip_lib):
    text = open(os.path.join(ROOT, "include", "raytrace_hip.h")).read()
    for name in ("rtHipSampleWindowCheck", "rtHipSceneSetSampleWindow", "rtHipSceneGetSampleWindow"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in R.RESIDENT_SYMBOLS
        assert hasattr(hip_lib, name), f"libraytrace_hip.so does not export {name}"
    assert "SAMPLE WINDOWS" in text and text.index("SAMPLE WINDOWS") < text.index("VARIANCE-GUIDED FILTER")
    assert "One limit" not in text
    assert C.sizeof(R.SampleWindow) == 20
    assert [f[0] for f in R.SampleWindow._fields_] == ["total", "first", "divisor", "accumulate", "advance"]
    for method in ("set_sample_window", "sample_window", "progressive"):
        assert callable(getattr(R.ResidentScene, method))


REFUSALS = WC.REFUSALS  # (samples, window, what the error text must say): shared with the session sequences


@pytest.mark.parametrize("samples, window, text", REFUSALS)
def test_every_refusal_has_its_own_text(samples, window, text):
    rc, err = check(samples, *window)
    assert rc == -1 and text in err, (rc, err)


def test_refusal_texts_are_distinct():
    """One text per rule: total, divisor, range, accumulate, advance flag, advance with N % S, advance with f % S."""
    picks = [REFUSALS[i] for i in (0, 1, 2, 5, 6, 8, 9)]
    texts = [re.sub(r"\d+", "#", check(s, *w)[1]) for s, w, _ in picks]
    assert len(set(texts)) == len(picks), texts


@pytest.mark.parametrize("samples, window", [
    (2, (2, 0, 2, 0, 0)),                      # the default window
    (2, (8, 6, 8, 1, 1)),                      # f + S == N
    (1, (U32_MAX, U32_MAX - 1, 1, 0, 0)),      # N = 2^32 - 1, f + S == N, D = 1
    (1, (U32_MAX, 0, U32_MAX, 1, 1)),          # every N is a multiple of S = 1
    (3, (4, 1, 4, 0, 0)),                      # a window that does not start on a multiple of S (no advance)
    (5, (5, 0, 1, 1, 0)),
])
def test_legal_edges_are_accepted(samples, window):
    rc, err = check(samples, *window)
    assert rc == 0, err


def test_null_arguments_are_refused_without_a_device(hip_lib):
    L = R.lib()
    assert L.rtHipSampleWindowCheck(2, None) == -1
    w = R.SampleWindow(2, 0, 2, 0, 0)
    assert L.rtHipSceneSetSampleWindow(None, C.byref(w)) == -1 and "null scene" in R.last_error()
    assert L.rtHipSceneGetSampleWindow(None, C.byref(w), None) == -1 and "null scene" in R.last_error()
    assert check(0, 1, 0, 1, 0, 0)[0] == -1  # (no scene has S = 0)


@pytest.mark.parametrize("name", sorted(WC.DIVISOR_SCENES))
def test_premises_of_the_divisor_test_hold_on_the_goldens(name):
    """The divisor test wants frames with enough lit values (>= 5 %) and next to no saturated ones (<= 1 %): the goldens of its
    one-sample scenes show 7.9 %, 10.7 % and 19.4 % non-zero and 0, 0.01 % and 0 saturated."""
    sc, planes = WC.golden(name)
    assert sc.sample_count == 1
    nonzero, saturated = WC.shares(planes)
    want_nonzero, want_saturated = WC.DIVISOR_SCENES[name]
    assert abs(nonzero - want_nonzero) < 0.0006, nonzero
    assert abs(saturated - want_saturated) < 0.00006, saturated
    assert nonzero >= 0.05 and saturated <= 0.01


def test_progressive_cases_name_goldens_with_the_stated_sample_counts():
    for name, samples, total in WC.PROGRESSIVE:
        sc, planes = WC.golden(name)
        assert sc.sample_count == samples and total % samples == 0 and total > samples
    # the case that proves the order of the saturating adds: 5.8 % of its golden is saturated and one light is negative
    sc, planes = WC.golden("degenerate_and_outside")
    assert abs(WC.shares(planes)[1] - 0.058) < 0.0006 and (sc.light_col[:, :3] < 0).any()
    # the golden of the scene of the off-grid windows shows no saturation
    assert WC.shares(WC.golden("lambert_distant")[1])[1] == 0.0


# ---- the window oracle (oracle_lib.oracle_render_window), tied to the goldens and to the oracle's N-sample frames -----------------------
THREADS = min(os.cpu_count() or 1, 16)


@pytest.mark.parametrize("name", golden_names())
def test_the_window_oracle_under_the_default_window_is_the_golden(name):
    sc, want = WC.golden(name)
    S = sc.sample_count
    got = O.oracle_render_window(sc, S, 0, S, threads=THREADS)
    assert WC.differing(got, want) == 0


@pytest.mark.parametrize("name, samples, total", WC.PROGRESSIVE)
def test_chained_windows_of_the_oracle_are_its_n_sample_frame(name, samples, total):
    """degenerate_and_outside (5.8 % saturated, one negative light) proves the order of the saturating adds."""
    sc, _ = WC.golden(name)
    chain = WC.window_chain(name, total)
    assert len(chain) == total // samples
    assert WC.differing(chain[-1], WC.oracle_frame(name, total)) == 0
    for a, b in zip(chain, chain[1:]):
        assert WC.differing(a, b) > 0  # (every window adds something)


def test_chained_windows_off_the_sample_grid_are_the_oracles_frame():
    """lambert_distant, N = 5: S = 2 at f = 0 and f = 2, then a one-sample scene at f = 4."""
    sc, _ = WC.golden("lambert_distant")
    assert sc.sample_count == 2
    planes = O.oracle_render_window(sc, 5, 0, 5, threads=THREADS)
    planes = O.oracle_render_window(sc, 5, 2, 5, onto=planes, threads=THREADS)
    planes = O.oracle_render_window(WC.with_samples(sc, 1), 5, 4, 5, onto=planes, threads=THREADS)
    assert WC.differing(planes, WC.oracle_frame("lambert_distant", 5)) == 0


def test_the_window_oracle_copies_what_it_adds_onto():
    sc, _ = WC.golden("lambert_distant")
    first = O.oracle_render_window(sc, 8, 0, 8, threads=THREADS)
    kept = [p.copy() for p in first]
    second = O.oracle_render_window(sc, 8, 2, 8, onto=first, threads=THREADS)
    assert WC.differing(first, kept) == 0 and WC.differing(second, first) > 0
    assert all((b >= a).all() for a, b in zip(first, second))  # (no negative light in this scene: the adds only raise)


def test_a_smaller_divisor_saturates_more():
    name, S, N = "degenerate_and_outside", 3, 12
    sc, _ = WC.golden(name)
    assert sc.sample_count == S
    full = O.oracle_render_window(sc, N, 3, N, threads=THREADS)
    half = O.oracle_render_window(sc, N, 3, N // 2, threads=THREADS)
    assert WC.shares(half)[1] > WC.shares(full)[1]
    assert sum(int((p == WC.SATURATED).sum()) for p in half) > sum(int((p == WC.SATURATED).sum()) for p in full)


def test_the_window_oracle_refuses_what_the_library_refuses():
    sc, _ = WC.golden("lambert_distant")
    planes = [np.zeros(sc.pixels, np.uint16) for _ in range(3)]
    osc = O.oracle_scene(sc, planes)
    for total, first, divisor in ((0, 0, 2), (8, 0, 0), (8, 7, 8), (U32_MAX, U32_MAX - 1, 1)):
        assert O.oracle().rt_oracle_render_window(C.byref(osc), total, first, divisor, 0, sc.pixels, 1) == 0
        assert check(sc.sample_count, total, first, divisor, 0, 0)[0] == -1
    assert not any(p.any() for p in planes)


def test_command_line_refusals_and_acceptance():
    from opencl_render_amd import __main__ as M
    for bad in (["--samples", "4", "--progressive", "6"],                  # N no multiple of S
                ["--samples", "4", "--progressive", "2"],                  # N < S
                ["--samples", "2", "--progressive", "8", "--orbit", "3"],
                ["--samples", "2", "--progressive", "8", "--spin", "3"],
                ["--samples", "2", "--progressive", "8", "--passes", "p"],
                ["--samples", "2", "--progressive", "8", "--denoise", "d.ppm"],
                ["--samples", "2", "--progressive", "8", "--ao", "a.pfm"],
                ["--samples", "2", "--progressive", "8", "--sequence", "8"],
                ["--samples", "2", "--sequence", "8"],                     # no frames to run the sequence over
                ["--samples", "2", "--sequence", "7", "--orbit", "3"],
                ["--samples", "4", "--sequence", "2", "--spin", "3"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)
    a = M.parse_args(["--samples", "2", "--progressive", "8"])
    assert (a.progressive, a.sequence) == (8, 0)
    a = M.parse_args(["--samples", "2", "--sequence", "8", "--orbit", "3", "--temporal", "acc.pfm"])
    assert (a.progressive, a.sequence) == (0, 8)
    assert M.parse_args([]).progressive == 0 and M.parse_args([]).sequence == 0
