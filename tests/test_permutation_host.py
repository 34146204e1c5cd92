"""CPU: ``jumpy.random_permutation`` on host keys against the oracle's threefry (oracle/pob_np.py
``split`` and ``random_bits``) with numpy's stable argsort, spelled out here: rounds = ceil(3 ln n /
ln(2^32 - 1)); per round ``key, sub = split(key)`` and x <- x stably sorted by ``random_bits(sub, n)``.

n covers no round (1), one (2, 64, 1 625), and two (1 626, 4 096).  The scheme is [ext], recalled; what
is already pinned is the reset kernels' ``choice``, and for n = 156 the first 16 entries
must be the oracle's ``choice_noreplace``.  Stability: PRNGKey(179) draws one pair of equal sort words
in round 0 at n = 4 096 and PRNGKey(16) one in round 1 (found by searching seeds 0 .. 999 with the
oracle; about 0.2 % of the keys a round), so an unstable sort shows there."""
import numpy as np
import pytest
import torch

import pob_np as P

NS = [1, 2, 64, 1625, 1626, 4096]
DUPLICATE_SEEDS = [(179, 0), (16, 1)]  # (seed, the round whose words hold one equal pair) at n = 4096


def rounds_of(n):
    return int(np.ceil(3 * np.log(max(1, n)) / np.log(2 ** 32 - 1)))


def oracle_permutation(key, n):
    """(x, [the words of every round])"""
    x, words = np.arange(n), []
    for _ in range(rounds_of(n)):
        key, sub = P.split(key)
        w = P.random_bits(sub, n)
        words.append(w)
        x = x[np.argsort(w, kind="stable")]
    return x, words


def tkey(key):
    return torch.from_numpy(np.asarray(key, np.uint32).astype(np.int64)).to(torch.uint32)


def test_round_counts():
    from po_brax_amd import jumpy
    assert [jumpy.permutation_rounds(n) for n in (1, 2, 1625, 1626, 2642245, 2642246)] == [0, 1, 1, 2, 2, 3]
    assert [rounds_of(n) for n in NS] == [0, 1, 1, 1, 2, 2]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("seed", [0, 7])
def test_against_the_oracle(n, seed):
    from po_brax_amd import jumpy
    key = P.prngkey(seed)
    want, _ = oracle_permutation(key, n)
    tk = tkey(key)
    got = jumpy.random_permutation(tk, n)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n,) and got.device.type == "cpu"
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(np.sort(got.numpy()), np.arange(n))
    assert np.array_equal(tk.numpy(), np.asarray(key, np.uint32))  # the key is only read
    if n == 1:
        assert got.tolist() == [0]
    else:
        assert not np.array_equal(want, np.arange(n))


def test_equals_the_pinned_choice():
    from po_brax_amd import jumpy
    for seed in range(4):
        key = P.prngkey(seed)
        got = jumpy.random_permutation(tkey(key), 156)[:16].numpy()
        assert np.array_equal(got, P.choice_noreplace(key, np.arange(156), 16))
        assert np.array_equal(got, P.permutation_indices(key, 156)[:16])


@pytest.mark.parametrize("seed,dup_round", DUPLICATE_SEEDS)
def test_equal_sort_words_keep_their_order(seed, dup_round):
    from po_brax_amd import jumpy
    n = 4096
    key = P.prngkey(seed)
    want, words = oracle_permutation(key, n)
    assert [n - np.unique(w).size for w in words] == [int(r == dup_round) for r in range(2)]  # the pinned collision
    # an unstable order of the equal pair gives another permutation: the case can tell
    w = words[dup_round]
    order = np.argsort(w, kind="stable")
    i = int(np.flatnonzero(w[order][1:] == w[order][:-1])[0])
    swapped = order.copy()
    swapped[[i, i + 1]] = swapped[[i + 1, i]]
    assert not np.array_equal(order, swapped) and order[i] < order[i + 1]
    got = jumpy.random_permutation(tkey(key), n).numpy()
    assert np.array_equal(got, want)


def test_host_bits_are_the_oracles():
    from po_brax_amd.training import networks
    for n in (1, 2, 5, 64):
        key = P.prngkey(3)
        assert np.array_equal(networks._host_bits(tkey(key), n).numpy().astype(np.uint32), P.random_bits(key, n))


def test_arguments():
    from po_brax_amd import jumpy
    with pytest.raises(ValueError):
        jumpy.random_permutation(tkey(P.prngkey(0)), 0)
    with pytest.raises(TypeError):
        jumpy.random_permutation(torch.zeros(2, dtype=torch.int32), 4)
