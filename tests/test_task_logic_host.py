"""CPU: the C oracle's task logic against what the reference's own code returned
(tests/golden/task_logic_*.npz, tests/task_cases.py): reset sampling, observation assembly,
rewards, done, metrics, the TAG adversary, the GA sensor bins, the wall tables and the
autoreset wrappers, bit for bit.  The kernels are held to the same files by
tests/test_gpu_task_logic.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import orc
import task_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
# the reference checkout: $PO_BRAX_REFERENCE, or a directory "reference" beside this repository
REFERENCE = [p for p in (os.environ.get("PO_BRAX_REFERENCE"), os.path.join(HERE, "..", "..", "reference"))
             if p and os.path.isdir(os.path.join(p, "po_brax", "envs"))]


@pytest.fixture(scope="module", params=TC.KINDS)
def case(request):
    return request.param, TC.load(request.param), orc.OracleEnv(request.param)


def test_fixture_files_are_small_data():
    for kind in TC.KINDS:
        assert os.path.getsize(TC.path(kind)) < 200_000, kind
        for k, v in TC.load(kind).items():
            assert v.dtype.kind in "fiu", (kind, k, v.dtype)


def test_events_present(case):
    """every branch the issue lists is in the files, with its opposite, at least 4 times"""
    kind, fix, _ = case
    n = TC.assert_events(kind, fix)
    print(kind, n)


def test_oracle_reset_matches_reference(case):
    kind, fix, o = case
    s = o.reset(TC.keys(fix["reset_seed"], TC.N_RESET))
    TC.compare_reset(kind, s, fix, f"{kind} oracle reset")
    assert not s["reward"].any() and not s["done"].any() and not (s["m0"].any() or s["m1"].any() or s["m2"].any())


def test_oracle_step_matches_reference(case):
    kind, fix, o = case
    base = o.reset(TC.keys(fix["step_seed"], TC.B_STEP))
    out = o.step(TC.arrange(kind, base, fix), fix["step_act"], flags=0)
    # the reference's observation starts with the torso the placements were searched for
    TC.compare_step(kind, TC.oracle_step_outputs(kind, out), fix, f"{kind} oracle step")


def test_oracle_last_sensor_slot_matches_reference():
    """ten apples and six bombs: a bomb's reading in the last slot, kept or zeroed by a later
    object without a bin (the -1 wrap), which the default eight and eight cannot produce"""
    fix = TC.load(TC.GA)
    o = orc.OracleEnv(TC.GA, **{"ga_" + k: v for k, v in TC.ALT_PARAMS.items()})
    base = o.reset(TC.keys(fix["alt_seed"], TC.B_ALT))
    out = o.step(TC.arrange(TC.GA, base, fix, "alt"), fix["alt_act"], flags=0)
    TC.compare_step(TC.GA, TC.oracle_step_outputs(TC.GA, out), fix, "ant_gather ten apples", "alt")


def test_walls_match_reference(case):
    """draw_arena / draw_t_maze as the reference computes them against the oracle's wall boxes
    and the exported brax config, bit for bit: centres, half sizes, the exported angle (float32),
    and the oracle's cos / sin against the float32 cos / sin of the reference's angle."""
    import ctypes as C
    from po_brax_amd import _lib
    from po_brax_amd.io.config import brax_config_of
    kind, fix, o = case
    w, ref = o.walls(), fix["walls"]
    assert len(w) == len(ref) == (8 if kind == TC.HH else 4)
    TC.same(w[:, [0, 1, 4, 5]], ref[:, [0, 1, 3, 4]], f"{kind} walls: centre, half size")
    rad = np.deg2rad(ref[:, 2].astype(np.float64))
    TC.same(w[:, 2], np.cos(rad).astype(np.float32), f"{kind} walls: cos")
    TC.same(w[:, 3], np.sin(rad).astype(np.float32), f"{kind} walls: sin")
    assert (ref[:, 5] == 0.5).all() and (ref[:, 6] == 0.5).all()
    p = _lib.pob_params()
    assert _lib.lib.pob_default_params(C.byref(p)) == 0
    arena = [b for b in brax_config_of(kind, p)["bodies"] if b["name"] == "Arena"][0]["colliders"]
    got = np.array([[c["position"]["x"], c["position"]["y"], c["rotation"]["z"], c["box"]["halfsize"]["x"],
                     c["box"]["halfsize"]["y"], c["box"]["halfsize"]["z"]] for c in arena], np.float32)
    TC.same(got, ref[:, :6], f"{kind} exported walls")


def _fix():
    return TC.load(TC.WRAP_KIND), orc.OracleEnv(TC.WRAP_KIND)


def test_wrapper_records_have_done_and_not_done():
    fix, _ = _fix()
    for name in ("naive", "cached", "gym"):
        d = fix[f"{name}_inner_done"]
        assert d.shape == (TC.WRAP_T, TC.WRAP_B)
        assert (d != 0).any(1).sum() >= 3 and (d == 0).any(1).all(), name


def test_oracle_naive_autoreset_matches_reference():
    fix, o = _fix()
    for t, (s, inner) in enumerate(TC.oracle_naive(o, *TC.wrap_inputs(fix))):
        TC.compare_wrap("naive", t, s, fix, "naive")
        TC.same(inner, fix["naive_inner_done"][t], f"naive step {t}: inner done")


def test_oracle_cached_autoreset_matches_reference():
    fix, o = _fix()
    for t, (s, _) in enumerate(TC.oracle_cached(o, *TC.wrap_inputs(fix))):
        TC.compare_wrap("cached", t, s, fix, "cached")
        TC.same(s["first_obs"], fix["cached_first_obs"][t], f"cached step {t}: first_obs")
        TC.same(s["first_pos"], fix["cached_first_pos"][t], f"cached step {t}: first_qp.pos")


def test_oracle_gym_autoreset_matches_reference():
    fix, o = _fix()
    _, steps0, acts = TC.wrap_inputs(fix)
    for t, (s, inner, gkey) in enumerate(TC.oracle_gym(o, steps0, acts)):
        TC.compare_wrap("gym", t, s, fix, "gym")
        TC.same(inner, fix["gym_inner_done"][t], f"gym step {t}: inner done")
        TC.same(gkey, fix["gym_key"][t], f"gym step {t}: gym key")


@pytest.mark.skipif(not REFERENCE, reason="the reference checkout is not on this machine")
def test_fixtures_are_current(tmp_path):
    """the maker, run on the reference tree, writes what is committed: every member's name,
    type, shape and bytes (the archive's own bytes carry the zip's timestamps)"""
    run = subprocess.run([sys.executable, os.path.join(HERE, "golden", "make_task_logic_fixture.py"), REFERENCE[0],
                          "--out", str(tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    for kind in TC.KINDS:
        new, old = TC.load(kind, os.path.join(tmp_path, os.path.basename(TC.path(kind)))), TC.load(kind)
        assert sorted(new) == sorted(old), kind
        for k in old:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, (kind, k)
            assert new[k].tobytes() == old[k].tobytes(), (kind, k)
