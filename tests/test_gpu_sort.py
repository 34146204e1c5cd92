"""GPU: the engine's stable radix sort (``jumpy.stable_argsort`` / ``pob_sort_pairs_u32``) against numpy's
stable argsort on uint32, ``jumpy.random_permutation(key, n, sort="native")`` against the CPU-key path
(test_permutation_host.py holds that one to the oracle), and ``PPOLearner(permutation="native")``
against ``"threefry"``.  Every comparison is exact; outputs and workspaces start from a sentinel.

TILE = 2 048 (POB_SORT_TILE: 256 lanes x 8 items).  k_sort_scan walks a digit's row of tile counts
POB_SORT_SCAN_CHUNK = 256 tiles at a time, so n = 256 x 2 048 + 1 is the smallest n with a second chunk."""
import numpy as np
import pytest
import torch

import pob_np as P
import test_gpu_learner as ff
import learner_ref as ref
from test_permutation_host import DUPLICATE_SEEDS, tkey

pytestmark = pytest.mark.gpu

TILE, SCAN_CHUNK = 2048, 256
MULTI = 3 * TILE + 1
CHUNKS = SCAN_CHUNK * TILE + 1
SIZES = [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, MULTI, CHUNKS]
EDGES = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)
FAMILIES = {
    "uniform": lambda rng, n: rng.integers(0, 2 ** 32, n, dtype=np.uint32),
    "equal": lambda rng, n: np.full(n, 0xDEADBEEF, np.uint32),
    "edges": lambda rng, n: EDGES[rng.integers(0, 5, n)],
    "byte0": lambda rng, n: np.uint32(0x5A5A5A00) | rng.integers(0, 256, n, dtype=np.uint32),
    "byte1": lambda rng, n: np.uint32(0x5A5A005A) | (rng.integers(0, 256, n, dtype=np.uint32) << 8),
    "byte2": lambda rng, n: np.uint32(0x5A005A5A) | (rng.integers(0, 256, n, dtype=np.uint32) << 16),
    "byte3": lambda rng, n: np.uint32(0x005A5A5A) | (rng.integers(0, 256, n, dtype=np.uint32) << 24),
    "ascending": lambda rng, n: np.sort(rng.integers(0, 2 ** 32, n, dtype=np.uint32)),
    "descending": lambda rng, n: np.sort(rng.integers(0, 2 ** 32, n, dtype=np.uint32))[::-1].copy(),
}
CASES = [("uniform", n) for n in SIZES] + [(f, MULTI) for f in FAMILIES if f != "uniform"] + [("edges", CHUNKS)]


def _buffers(n):
    from po_brax_amd import jumpy
    out = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    return out, jumpy.sort_workspace(n, "cuda").fill_(0xA5)


@pytest.mark.parametrize("family,n", CASES)
def test_stable_argsort(family, n):
    from po_brax_amd import jumpy
    words = FAMILIES[family](np.random.default_rng(n), n)
    out, ws = _buffers(n)
    got = jumpy.stable_argsort(torch.from_numpy(words).cuda(), out=out, workspace=ws)
    assert got is out
    assert np.array_equal(got.cpu().numpy(), np.argsort(words, kind="stable").astype(np.int32))


def test_sort_pairs_with_a_payload():
    from po_brax_amd import _lib
    rng = np.random.default_rng(5)
    words, vals = FAMILIES["edges"](rng, MULTI), rng.integers(-2 ** 31, 2 ** 31, MULTI).astype(np.int32)
    k, v = torch.from_numpy(words).cuda(), torch.from_numpy(vals).cuda()
    out, ws = _buffers(MULTI)
    k_out = torch.zeros_like(k)
    _lib.check(_lib.lib.pob_sort_pairs_u32(k.data_ptr(), v.data_ptr(), MULTI, k_out.data_ptr(), out.data_ptr(), ws.data_ptr(),
                                           ws.numel(), _lib.stream_handle(k.device)))
    order = np.argsort(words, kind="stable")
    assert np.array_equal(k_out.cpu().numpy(), words[order]) and np.array_equal(out.cpu().numpy(), vals[order])


@pytest.mark.parametrize("seed,n", [(0, 1), (0, 2), (7, 156), (0, 1625), (0, 1626), (7, MULTI)]
                         + [(seed, 4096) for seed, _ in DUPLICATE_SEEDS])
def test_native_permutation_equals_the_host_path(seed, n):
    from po_brax_amd import jumpy
    key = tkey(P.prngkey(seed))
    dkey = key.cuda()
    got = jumpy.random_permutation(dkey, n, sort="native")
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (n,)
    assert torch.equal(got.cpu(), jumpy.random_permutation(key, n))
    assert torch.equal(dkey.cpu(), key)  # the key is only read


def test_native_permutation_through_a_reused_workspace():
    from po_brax_amd import jumpy
    out, ws = _buffers(MULTI)
    for seed in (3, 4):  # the second call finds the first one's tables and pairs in the workspace
        key = tkey(P.prngkey(seed))
        got = jumpy.random_permutation(key.cuda(), MULTI, sort="native", workspace=ws, out=out)
        assert got is out and torch.equal(got.cpu(), jumpy.random_permutation(key, MULTI))


def test_native_learner_equals_the_threefry_learner():
    """T x B = 4 x 64 in 4 minibatches x 2 epochs: n = 256 keeps the threefry leg on torch's small sort."""
    from po_brax_amd.training import PPOLearner
    thetas = []
    for permutation in ("threefry", "native"):
        rng = np.random.default_rng(0)
        norm = ff._loaded_normalizer(rng, ff.D)
        policy, value_fn = ff._actors(0, norm)
        roll = ref.make_roll(rng, 4, 64, ff.D, ff.A, policy, norm, 0.3, "cuda")
        learner = PPOLearner(policy, value_fn, learning_rate=3e-3, num_minibatches=4, num_update_epochs=2,
                             key=ff._key(300), backward="native", optimizer="fused", permutation=permutation)
        for _ in range(2):
            learner.update(roll)
        torch.cuda.synchronize()
        thetas.append([t.detach().clone() for t in learner._theta] + [learner.perm_key.clone()])
    assert learner._perm_workspace is not None
    for a, b in zip(*thetas):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
