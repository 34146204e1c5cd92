"""CPU: the per-body cut of a lane's contact slots in the four-lane kernel's block-cooperative
wall walk (po-brax_amd/csrc/pob_blockwalk.h bw_body_ranges, the header the kernel compiles),
driven on the host for four waves x 64 lanes (tests/host/body_ranges_host.cpp).  The position
and the velocity pass walk body l's slots [c[l], c[l + 1]) in a loop of their own, so for random
per-body counts -- zero, saturated and overflowing ones included --
  * the three ranges tile bw_apply_range's [c0, c1) exactly (checked in the host model, and
    against boundaries formed here from the masks' popcounts alone);
  * they follow the publish order: every slot of body l's range is an item of that lane on
    body l, the slots ascend in walk order (slot, bit, triangle), and the kernel's body-by-body
    publish writes the records the walk-order publish (bw_next_item) writes;
  * all four boundaries are equal in an overflowing block.
The same source builds as a stand-alone program (-DBR_MAIN), run here once under
-fsanitize=address,undefined (host code only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "body_ranges_host.cpp")
WAVES, WCAP, CAP, LANE_MAX = 4, 50, 200, 64  # QBW_WAVES, QBW_WCAP, QBW_CAP, QBW_LANE_MAX


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("br_host")
    so = d / "br_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-I", CSRC, "-shared", "-o", str(so), SRC])
    lib = C.CDLL(str(so))
    IP = C.POINTER(C.c_int)
    lib.br_substep.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, IP, IP]
    return lib


def _check(lib, masks, cap, dead_mask=0):
    masks = np.ascontiguousarray(masks, np.uint64)
    assert masks.shape == (WAVES, 64, 3)
    ranges = np.zeros((WAVES, 64, 4), np.int32)
    info = np.zeros(4, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.br_substep(masks.ctypes.data_as(C.POINTER(C.c_uint64)), cap, dead_mask, ip(ranges), ip(info))
    assert rc == 0, rc
    live = np.array([((dead_mask >> w) & 1) == 0 for w in range(WAVES)])
    pop = np.vectorize(lambda x: bin(int(x)).count("1"))(masks) * live[:, None, None]  # (waves, lanes, bodies)
    nl = np.minimum(pop.sum(-1), LANE_MAX)
    ovf = bool(nl.sum() > cap or (nl.sum(-1) > WCAP).any())
    assert bool(info[0]) == ovf, (info, nl.sum(-1), cap)
    assert info[1] == 1 and info[2] == 1 and info[3] == 1, info
    base = np.cumsum(nl, -1) - nl  # the items of the lanes below
    want = 2 * base[..., None] + (0 if ovf else 2) * np.concatenate([np.zeros_like(pop[..., :1]), np.cumsum(pop, -1)], -1)
    assert np.array_equal(ranges, want)
    if ovf:
        assert (ranges == ranges[..., :1]).all()  # collapsed: nothing to apply
    else:
        assert np.array_equal(ranges[..., 3] - ranges[..., 0], 2 * nl)
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
    rng = np.random.default_rng(11)
    n_ovf = 0
    for it in range(300):
        m = _random_masks(rng, rng.uniform(0.0, 0.04))
        n_ovf += _check(host, m, CAP if it % 3 else 16, 0xC if it % 10 == 9 else 0)
    assert 20 < n_ovf < 280, n_ovf  # both kinds occur


def test_zero_and_single_body_counts(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    assert not _check(host, z, CAP)
    for body in range(3):  # items on one body only: the other two ranges are empty
        m = z.copy()
        m[2, 9, body] = 0b1011 << 8
        m[2, 10, (body + 1) % 3] = 1
        assert not _check(host, m, CAP)
    m = z.copy()
    m[0, 0, 0] = 1 << 5; m[0, 0, 2] = 0b11 << 40       # torso and leg, no Aux
    m[0, 63, 1] = 0b111                                # three items of one body on the wave's last lane
    m[3, 1, :] = [1 << 47, 1 << 0, (1 << 47) | 1]      # all three bodies
    assert not _check(host, m, CAP)


def test_saturated_and_overflowing_counts(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    m = z.copy()
    m[1, 17, 1] = (1 << 30) - 1   # 30 items of one body
    m[1, 17, 2] = 0x7FFFF << 8    # + 19 of the next: 49 <= the segment
    m[1, 18, 0] = 1
    assert WCAP == 50 and not _check(host, m, CAP)
    m[1, 40, 0] = 0b11            # the wave's count 52 > its segment
    assert _check(host, m, CAP)
    m = z.copy()
    m[0, 5, :] = (1 << 48) - 1    # 144 items on one lane: the lane's count saturates, the wave overflows
    m[0, 6, 1] = 1
    m[2, 0, 2] = 0b101
    assert _check(host, m, CAP)
    m = z.copy()
    m[3, 7, 0] = (1 << 48) - 1    # 48 + 16 = 64: exactly the saturation value
    m[3, 7, 1] = (1 << 16) - 1
    assert _check(host, m, CAP)
    for cap in (16, 47):          # the block's capacity: the boundary on either side
        for total in (cap, cap + 1):
            m = z.copy()
            for i in range(total):
                m[i % WAVES, (i // WAVES) % 64, i % 3] |= np.uint64(1 << (i % 48))
            assert _check(host, m, cap) == (total > cap), (cap, total)


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "br_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DBR_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
