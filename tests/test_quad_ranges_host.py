"""CPU: "the torso's items once per lane quad" of the four-lane kernel's block-cooperative wall
walk (po-brax_amd/csrc/pob_blockwalk.h bw_quad_lead / bw_quad_torso_count / bw_quad_ranges, the
header the kernel compiles), driven on the host for four waves x 64 lanes
(tests/host/quad_ranges_host.cpp).  The four lanes of a quad hold the same torso, so only the
quad's lane 0 counts and publishes the torso's items and all four lanes apply the torso's
contacts from that lane's slots.  For random item masks -- the torso's equal within each quad,
heavy lanes, waves past the batch and a lowered capacity included --
  * lane 0 of a quad alone publishes torso records;
  * every lane's torso range is its quad lane 0's torso slots, in walk order;
  * every lane's own ranges enumerate its Aux, then its lower-leg items in walk order;
  * the union of all ranges covers each published contact slot exactly once per lane of the
    owning quad (a torso slot) or once (an Aux / lower-leg slot), and nothing else;
  * all ranges are empty in an overflowing block;
  * the prefix cut to two ballot steps when no lane of the wave holds four items or more gives
    the bases and totals of all seven steps.
The ranges are also formed here from the masks' popcounts alone.  The same source builds as a
stand-alone program (-DQR_MAIN), run here once under -fsanitize=address,undefined (host code
only)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "po-brax_amd", "csrc")
SRC = os.path.join(HERE, "host", "quad_ranges_host.cpp")
WAVES, WCAP, CAP, LANE_MAX = 4, 50, 200, 64  # QBW_WAVES, QBW_WCAP, QBW_CAP, QBW_LANE_MAX


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("qr_host")
    so = d / "qr_host.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-I", CSRC, "-shared", "-o", str(so), SRC])
    lib = C.CDLL(str(so))
    IP = C.POINTER(C.c_int)
    lib.qr_substep.argtypes = [C.POINTER(C.c_uint64), C.c_int, C.c_int, IP, IP, IP]
    return lib


def _pop(a):
    return np.vectorize(lambda x: bin(int(x)).count("1"))(a)


def _check(lib, masks, cap, dead_mask=0):
    masks = np.ascontiguousarray(masks, np.uint64)
    assert masks.shape == (WAVES, 64, 3)
    ranges = np.zeros((WAVES, 64, 5), np.int32)
    counts = np.zeros(WAVES, np.int32)
    info = np.zeros(6, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    rc = lib.qr_substep(masks.ctypes.data_as(C.POINTER(C.c_uint64)), cap, dead_mask, ip(ranges), ip(counts), ip(info))
    assert rc == 0, rc
    live = np.array([((dead_mask >> w) & 1) == 0 for w in range(WAVES)])
    pop = _pop(masks) * live[:, None, None]          # (waves, lanes, bodies)
    lead = (np.arange(64) & 3) == 0
    n0 = np.repeat(pop[:, ::4, 0], 4, axis=1)         # the quad's torso items: its lane 0's
    pub = pop.copy()
    pub[..., 0] = np.where(lead[None, :], n0, 0)      # what a lane publishes
    nl = np.minimum(pub.sum(-1), LANE_MAX)
    assert np.array_equal(counts, nl.sum(-1))
    ovf = bool(nl.sum() > cap or (nl.sum(-1) > WCAP).any())
    assert bool(info[0]) == ovf, (info, nl.sum(-1), cap)
    assert (info[1:] == 1).all(), info
    base = np.cumsum(nl, -1) - nl                     # the items of the lanes below
    base0 = np.repeat(base[:, ::4], 4, axis=1)
    k = 0 if ovf else 2
    want = np.stack([2 * base0, 2 * base0 + k * n0,
                     2 * (base + pub[..., 0]), 2 * (base + pub[..., 0]) + k * pop[..., 1],
                     2 * (base + pub[..., 0]) + k * (pop[..., 1] + pop[..., 2])], -1)
    assert np.array_equal(ranges, want)
    if ovf:
        assert (ranges[..., 0] == ranges[..., 1]).all() and (ranges[..., 2] == ranges[..., 4]).all()
    else:
        # a quad's four lanes read the same torso slots; lane 0's own ranges follow them
        assert np.array_equal(ranges[:, ::4, 1], ranges[:, ::4, 2])
        # items published = torso once per quad + every lane's own
        assert counts.sum() == pop[:, ::4, 0].sum() + pop[..., 1:].sum()
    return ovf


def _random_masks(rng, density):
    m = np.zeros((WAVES, 64, 3), np.uint64)
    on = rng.uniform(size=m.shape) < density
    bits = rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    bits &= rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    bits &= rng.integers(0, 1 << 48, size=m.shape, dtype=np.uint64)
    m[on] = bits[on]
    m[:, :, 0] = np.repeat(m[:, ::4, 0], 4, axis=1)   # the torso's mask: equal within a quad
    return m


def test_random_blocks(host):
    rng = np.random.default_rng(23)
    n_ovf = 0
    for it in range(300):
        m = _random_masks(rng, rng.uniform(0.0, 0.05))
        if it % 7 == 0:  # a heavy lane
            m[rng.integers(WAVES), rng.integers(64), 1 + rng.integers(2)] = np.uint64(rng.integers(0, 1 << 20))
        n_ovf += _check(host, m, CAP if it % 3 else 16, 0xC if it % 10 == 9 else 0)
    assert 20 < n_ovf < 280, n_ovf  # both kinds occur


def test_torso_cases(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    assert not _check(host, z, CAP)
    m = z.copy()
    m[1, 8:12, 0] = 0b101 << 16                        # the torso holds the quad's only items
    assert not _check(host, m, CAP)
    m[1, 10, 2] = 0b11                                 # + a leg of lane 2, none on lane 0's leg
    m[1, 7, 1] = 1; m[1, 12, 1] = 1 << 40              # neighbours on either side
    assert not _check(host, m, CAP)
    m[1, 8, 1] = 0b111 << 3; m[1, 8, 2] = 1            # lane 0: torso, Aux and leg at once
    assert not _check(host, m, CAP)
    m = z.copy()
    m[0, 60:64, 0] = (1 << 13) - 1                     # 13 torso items in the wave's last quad
    m[0, 63, 2] = 0b1111
    m[3, 0:4, 0] = 1 << 47
    assert not _check(host, m, CAP)
    m = z.copy()
    m[2, 21, 0] = 0b11                                 # a torso mask in a lane that is not the quad's lane 0: ignored
    m[2, 21, 1] = 1
    assert not _check(host, m, CAP)
    m = z.copy()
    m[0, 0:4, 0] = 1; m[1, 0:4, 0] = 1                 # waves 1 .. 3 past the batch
    assert not _check(host, m, CAP, dead_mask=0xE)


def test_capacity_boundaries(host):
    z = np.zeros((WAVES, 64, 3), np.uint64)
    m = z.copy()
    m[1, 16:20, 0] = (1 << 30) - 1                     # 30 torso items, once: with the three other lanes' it would be 120
    m[1, 17, 2] = 0x7FFFF << 8                         # + 19: 49 <= the segment
    m[1, 40, 1] = 1                                    # 50: the segment's last slot
    assert WCAP == 50 and not _check(host, m, CAP)
    m[1, 41, 1] = 1                                    # 51 > the segment
    assert _check(host, m, CAP)
    m = z.copy()
    m[3, 4:8, 0] = (1 << 48) - 1                       # 48 + 16 on the quad's lane 0: the saturation value
    m[3, 4, 1] = (1 << 16) - 1
    assert _check(host, m, CAP)
    for cap in (16, 47):                               # torso items count once towards the block's capacity
        for total in (cap, cap + 1):
            m = z.copy()
            for i in range(total):
                w, q = i % WAVES, (i // WAVES) % 16
                if i % 3 == 0:
                    m[w, 4 * q:4 * q + 4, 0] |= np.uint64(1 << (i % 48))
                else:
                    m[w, 4 * q + i % 4, 1 + i % 2] |= np.uint64(1 << (i % 48))
            assert _check(host, m, cap) == (total > cap), (cap, total)


def test_standalone_under_sanitizers(tmp_path):
    exe = tmp_path / "qr_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-DQR_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), SRC])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
