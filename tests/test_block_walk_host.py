"""CPU: the dealing arithmetic of the four-lane kernel's block-cooperative wall walk
(po-brax_amd/csrc/pob_blockwalk.h, the header the kernel compiles) driven on the host for four
waves x 64 lanes (tests/host/block_walk_host.cpp): the per-wave offsets, item -> (round, wave,
group), the (item, triangle) contact slot and the owner's enumeration.  Checked against counts
formed here from the masks alone:
  * every published item is evaluated exactly once (and nothing else is);
  * each owner enumerates its (slot, bit, triangle) in strictly ascending order, its items in
    its walk order, every one of its contact slots written;
  * every wave passes the same number of block barriers, whatever its items, a wave past the
    batch or an overflow;
  * overflow is flagged exactly when the block's count exceeds the capacity or a wave's count
    its segment.
The same source builds as a stand-alone program (-DBW_MAIN), run here once under
-fsanitize=address,undefined (host code only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "block_walk_host.cpp")
WAVES, WCAP, CAP, LANE_MAX = 4, 50, 200, 64  # QBW_WAVES, QBW_WCAP, QBW_CAP, QBW_LANE_MAX


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bw_host")
    so = d / "bw_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-I", CSRC, "-shared", "-o", str(so), SRC])
    lib = C.CDLL(str(so))
    IP = C.POINTER(C.c_int)
    lib.bw_substep.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, C.c_int, IP, IP, IP, IP, IP]
    return lib


def _run(lib, masks, cap, sub, dead_mask):
    masks = np.ascontiguousarray(masks, np.uint64)
    assert masks.shape == (WAVES, 64, 3)
    n_wave = np.zeros(WAVES, np.int32)
    evals = np.zeros((WAVES, WCAP), np.int32)
    rounds = np.zeros(WAVES, np.int32)
    barriers = np.zeros(WAVES, np.int32)
    info = np.zeros(4, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.bw_substep(masks.ctypes.data_as(C.POINTER(C.c_uint64)), cap, sub, dead_mask, ip(n_wave), ip(evals),
                        ip(rounds), ip(barriers), ip(info))
    assert rc == 0, rc
    return n_wave, evals, rounds, barriers, info


def _check(lib, masks, cap, sub, dead_mask=0):
    n_wave, evals, rounds, barriers, info = _run(lib, masks, cap, sub, dead_mask)
    live = np.array([((dead_mask >> w) & 1) == 0 for w in range(WAVES)])
    pop = np.vectorize(lambda x: bin(int(x)).count("1"))(masks).sum(-1)  # (waves, lanes)
    want = np.where(live, np.minimum(pop, LANE_MAX).sum(-1), 0)
    assert np.array_equal(n_wave, want), (n_wave, want)
    ovf = bool(want.sum() > cap or (want > WCAP).any())
    assert bool(info[1]) == ovf, (info, want, cap)
    assert info[0] == (0 if ovf else want.sum())
    assert info[2] == 1 and info[3] == 1, info
    assert np.array_equal(barriers, np.full(WAVES, 2)), barriers
    for w in range(WAVES):
        exp = np.zeros(WCAP, np.int32)
        if not ovf:
            exp[:want[w]] = 1
        assert np.array_equal(evals[w], exp), (w, evals[w], want)
    # the rounds are dealt evenly: wave w takes r = (w + sub) mod 4, + 4, ..
    R = 0 if ovf else -(-int(want.sum()) // 8)
    exp_r = [len(range((w + sub) % 4, R, 4)) for w in range(WAVES)]
    assert list(rounds) == exp_r and sum(exp_r) == R
    return ovf


def _random_masks(rng, density):
    m = np.zeros((WAVES, 64, 3), np.uint64)
    on = rng.uniform(size=m.shape) < density
    bits = rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    bits &= rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    bits &= rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    m[on] = bits[on]
    return m


def test_random_blocks(host):
    rng = np.random.default_rng(7)
    n_ovf = 0
    for it in range(300):
        m = _random_masks(rng, rng.uniform(0.0, 0.04))
        n_ovf += _check(host, m, CAP if it % 3 else 16, it % 5)
    assert 20 < n_ovf < 280, n_ovf  # both kinds occur


def test_empty_and_dead_waves(host):
    rng = np.random.default_rng(8)
    z = np.zeros((WAVES, 64, 3), np.uint64)
    assert not _check(host, z, CAP, 0)
    for dead in (0x0, 0xE, 0xC, 0x8):  # the ragged last block: waves past the batch
        for sub in range(5):
            m = _random_masks(rng, 0.02)
            m[2] = 0  # an empty live wave
            _check(host, m, CAP, sub, dead)


def test_one_lane_holding_many_items(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    m = z.copy()
    m[1, 17, 1] = (1 << 30) - 1   # 30 items of one body
    m[1, 17, 2] = 0x7FFFF << 8    # + 19 of the next: 49 <= the segment
    m[3, 63, 0] = 1 << 47
    assert WCAP == 50 and not _check(host, m, CAP, 3)
    m[1, 40, 0] = 0b11            # the wave's count 51 > its segment
    assert _check(host, m, CAP, 3)
    m = z.copy()
    m[0, 5, :] = (1 << 48) - 1    # 144 items on one lane: the lane's count saturates, the wave overflows
    assert _check(host, m, CAP, 1)


def test_totals_around_the_capacity(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    for cap in (16, 47, CAP):
        for total in (cap - 1, cap, cap + 1):
            m = z.copy()
            for i in range(total):  # one item per lane and body slot, dealt over the waves
                m[i % WAVES, (i // WAVES) % 64, 2 - (i // WAVES) // 64] |= np.uint64(1 << (i % 48))
            assert _check(host, m, cap, 2) == (total > cap), (cap, total)


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "bw_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DBW_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
