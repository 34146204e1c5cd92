"""CPU: the oracle's contact record (orc_contacts_record: wall contacts per env, collide substep
and dynamic body) against the oracle's own contact statistics, on envs far from every wall, and
its promise to change no output of orc_step."""
import ctypes as C

import numpy as np
import pytest

import orc
import wall_arrange as WA

NAMES = ["ant_heavenhell", "ant_gather", "ant_tag"]
B = 96


def _walled_state(name):
    """reset, then two ants of three onto points within 1.0 of a wall and every third one 3 m clear"""
    o = orc.OracleEnv(name)
    s = o.reset(WA.keys(B, 21), first=True)
    walls = o.walls()
    lo, hi = WA.arena_box(walls)
    rng = np.random.default_rng(4)
    cand = rng.uniform(lo - 5.0, hi + 5.0, (256 * B, 2))
    d = WA.wall_distance(cand, walls)
    xy = cand[d < 1.0][:B].astype(np.float32)
    clear = np.arange(B) % 3 == 2
    xy[clear] = cand[d >= 3.25][: clear.sum()]
    assert (WA.wall_distance(xy[clear], walls) >= 3.0).all()
    return o, WA.place(s, xy - s["pos"][:, 0, :2]), clear


@pytest.mark.parametrize("name", NAMES)
def test_record_matches_contact_stats(name):
    o, s, clear = _walled_state(name)
    act = WA.actions(B, 8, 1)[0]
    st = (C.c_longlong * 16)()
    o._L.orc_contact_stats(st)  # (zeroes the counters)
    o._L.orc_contact_stats_enable(1)
    try:
        _, rec = WA.record(o, s, act)
        o._L.orc_contact_stats(st)
    finally:
        o._L.orc_contact_stats_enable(0)
    assert rec.shape == (B, WA.NSUB, 9)
    assert rec.sum() > 0
    assert rec.sum() == st[2], (rec.sum(), st[2])          # triangle contacts
    assert rec.max() == st[4], (rec.max(), st[4])          # the most of one capsule in one detection
    assert (rec > 0).sum() == st[3]                        # capsule-substeps with a contact
    assert st[7] == B * WA.NSUB                            # detections: every collide substep recorded
    assert rec[clear].sum() == 0 and rec[~clear].sum() > 0


@pytest.mark.parametrize("name", NAMES + ["ant"])
def test_record_changes_no_output(name):
    if name == "ant":
        o = orc.OracleEnv(name)
        s = o.reset(WA.keys(B, 21), first=True)
    else:
        o, s, _ = _walled_state(name)
    for t, act in enumerate(WA.actions(B, 8, 3)):
        off = o.step(s, act, flags=WA.FLAGS, episode_length=2)
        on, rec = o.step_recorded(s, act, WA.NSUB, flags=WA.FLAGS, episode_length=2)
        assert off.keys() == on.keys()
        for k in off:
            np.testing.assert_array_equal(off[k].view(np.uint32), on[k].view(np.uint32), err_msg=f"{name} step {t}: {k}")
        if name == "ant":
            assert rec.sum() == 0  # (no walls)
        s = off


def test_record_off_writes_nothing():
    o, s, _ = _walled_state("ant_tag")
    act = WA.actions(B, 8, 1)[0]
    buf = np.full((B, WA.NSUB, 9), -7, np.int32)
    o._L.orc_contacts_record(buf.ctypes.data_as(C.POINTER(C.c_int)), WA.NSUB)
    o._L.orc_contacts_record(None, 0)
    o.step(s, act, flags=WA.FLAGS)
    assert (buf == -7).all()
