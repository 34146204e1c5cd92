"""CPU: the radix sort's entry points refuse bad arguments before any HIP call, the Python keywords refuse
unknown names, ``stable_argsort`` on a CPU tensor is numpy's stable argsort, and the workspace layout
(tests/host/sort_layout_host.cpp, a stand-alone program) holds under -fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "po-brax_amd", "csrc")
P = 0x10000  # stands for a device pointer: the checks fail before anything reads it


@pytest.mark.parametrize("args,message", [
    ((None, None, 8, P, P, P, 1 << 20, None), "NULL"),
    ((P, None, 8, P, None, P, 1 << 20, None), "NULL"),
    ((P, None, 8, P, P, None, 1 << 20, None), "workspace is NULL"),
    ((P, None, 0, P, P, P, 1 << 20, None), "n must be"),
    ((P, None, 1 << 31, P, P, P, 1 << 20, None), "n must be"),
    ((P, None, 8, P, P, P, 1023, None), "workspace of 1023 bytes"),
    ((P, P + 2, 8, P, P, P, 1 << 20, None), "aligned"),
])
def test_sort_pairs_refuses(args, message):
    from po_brax_amd import _lib
    with pytest.raises(ValueError, match=message):
        _lib.check(_lib.lib.pob_sort_pairs_u32(*args))


@pytest.mark.parametrize("args,message", [
    ((None, 8, P, P, 1 << 20, None), "NULL"),
    ((P, 8, None, P, 1 << 20, None), "NULL"),
    ((P, 8, P, None, 1 << 20, None), "workspace is NULL"),
    ((P, 0, P, P, 1 << 20, None), "n must be"),
    ((P, 8, P, P, 0, None), "workspace of 0 bytes"),
    ((P, 8, P, P + 1, 1 << 20, None), "aligned"),
])
def test_random_permutation_refuses(args, message):
    from po_brax_amd import _lib
    with pytest.raises(ValueError, match=message):
        _lib.check(_lib.lib.pob_random_permutation(*args))


def test_workspace_bytes():
    from po_brax_amd import _lib
    ns = [1, 2, 2047, 2048, 2049, 6145, 524289, 1310720, 2 ** 31 - 1]
    sizes = [_lib.lib.pob_sort_workspace_bytes(n) for n in ns]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[-1] > 16 * (2 ** 31 - 1)
    assert _lib.lib.pob_sort_workspace_bytes(0) < 0 and _lib.lib.pob_sort_workspace_bytes(2 ** 31) < 0


def test_unknown_names_raise():
    import test_learner_host as ff
    from po_brax_amd import jumpy
    from po_brax_amd.training import PPOLearner
    with pytest.raises(ValueError, match="sort must be"):
        jumpy.random_permutation(torch.tensor([0, 1], dtype=torch.uint32), 8, sort="bogus")
    policy, value_fn = ff.stub_actors(0, None, None)
    with pytest.raises(ValueError, match="permutation must be"):
        PPOLearner(policy, value_fn, key=ff._key(1), permutation="bogus")
    assert PPOLearner(policy, value_fn, key=ff._key(1), permutation="native").perm_key is not None


@pytest.mark.parametrize("n", [1, 65, 4097])
def test_stable_argsort_on_a_cpu_tensor(n):
    from po_brax_amd import jumpy
    words = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF], np.uint32)[np.random.default_rng(n).integers(0, 5, n)]
    got = jumpy.stable_argsort(torch.from_numpy(words))
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), np.argsort(words, kind="stable"))


def test_layout_program_under_sanitizers(tmp_path):
    exe = tmp_path / "sort_layout"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "host", "sort_layout_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "cases OK" in out.stdout
