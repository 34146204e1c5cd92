"""GPU: ``jumpy.random_bits`` and ``jumpy.random_permutation`` on device keys against the host path
(test_permutation_host.py holds that one to the oracle), for n with no, one and two sort rounds and
for the two pinned keys whose sort words hold an equal pair at n = 4 096 (the stable order)."""
import numpy as np
import pytest
import torch

import pob_np as P
from test_permutation_host import DUPLICATE_SEEDS, NS, oracle_permutation, tkey

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 2, 5, 64, 1625, 4096])
def test_random_bits(n):
    from po_brax_amd import jumpy
    key = P.prngkey(3)
    got = jumpy.random_bits(tkey(key).cuda(), n)
    assert got.dtype == torch.uint32 and tuple(got.shape) == (n,)
    assert np.array_equal(got.cpu().numpy(), P.random_bits(key, n))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed", [0, 7])
def test_device_path_equals_host_path(n, seed):
    from po_brax_amd import jumpy
    key = tkey(P.prngkey(seed))
    dkey = key.cuda()
    got = jumpy.random_permutation(dkey, n)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (n,)
    assert torch.equal(got.cpu(), jumpy.random_permutation(key, n))
    assert torch.equal(dkey.cpu(), key)  # the key is only read


@pytest.mark.parametrize("seed,dup_round", DUPLICATE_SEEDS)
def test_equal_sort_words_keep_their_order(seed, dup_round):
    from po_brax_amd import jumpy
    key = P.prngkey(seed)
    want, words = oracle_permutation(key, 4096)
    assert 4096 - np.unique(words[dup_round]).size == 1
    got = jumpy.random_permutation(tkey(key).cuda(), 4096)
    assert np.array_equal(got.cpu().numpy(), want)
