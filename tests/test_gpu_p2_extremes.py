"""GPU parity tests (run with -m gpu on an MI355X) of the FP64 Poseidon2 at the states and matrices whose words are the
largest and the smallest there are: the S-box keeps x^3 and x^4 only partially reduced (csrc/poseidon2_f64.cuh), and its
exactness rests on magnitude bounds that constant extreme inputs press hardest.  Word for word against the CPU oracle;
random data at every dispatch boundary is test_gpu_commit_dispatch.py's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
P = 2013265921


@pytest.fixture(scope="module")
def gpu():
    import torch
    from dvt_circuits_amd import capi

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    p = capi.Prover()
    yield p
    p.close()


# (stage calls run on the prover's stream, torch on its own: see test_gpu_commit_dispatch.py)
def dev(a):
    import torch

    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()
    torch.cuda.synchronize()
    return t


def filled(words, value=0):
    import torch

    t = torch.full((words,), value, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return t


def host(t):
    return t.cpu().numpy().view(np.uint32)


def gpu_permute(gpu, states, times=1):
    t = dev(states)
    gpu.to_internal(t)
    for _ in range(times):
        gpu.poseidon2_permute(t)
    gpu.from_internal(t)
    gpu.sync()
    return host(t).reshape(-1, 16)


def test_permute_extreme_states(gpu, oracle):
    s = np.zeros((3 + 16, 16), np.uint32)
    s[1] = P - 1
    s[2, 0::2] = (P - 1) // 2
    s[2, 1::2] = (P + 1) // 2
    for i in range(16):
        s[3 + i, i] = P - 1
    got = gpu_permute(gpu, s)
    for i in range(s.shape[0]):
        want = oracle.permute(s[i])
        assert (got[i] == want).all(), f"state {i} ({s[i].tolist()}): {got[i].tolist()} != {want.tolist()}"


def test_permute_random_states_chained(gpu, oracle):
    rng = np.random.default_rng(77)
    s = rng.integers(0, P, (4096, 16), dtype=np.uint32)
    got = gpu_permute(gpu, s, times=3)
    for i in range(s.shape[0]):
        want = oracle.permute(oracle.permute(oracle.permute(s[i])))
        assert (got[i] == want).all(), f"state {i}: {got[i].tolist()} != {want.tolist()}"


# [(width, log_height)], by the dispatch constants that test_gpu_commit_dispatch.py names:
#   [(9,14),(17,10)]  2^14 rows are one row per thread, 9 words = a whole block and a ragged one; the 2^10 x 17 segment is a
#                     coop row sponge of three blocks (chain_us = 27 > work_us = 5.1), injected by the coop level kernel
#   [(8,13)]          the tree starts at the coop levels
#   [(1,6)]           the top kernel alone
#   [(1,16),(9,14)]   levels of more than 2^13 nodes, which the trees above do not have: level 15 is
#                     merkle_level_kernel<false>, level 14 merkle_level_kernel<true> with the 2^14 x 9 rows injected
SHAPES = [[(9, 14), (17, 10)], [(8, 13)], [(1, 6)], [(1, 16), (9, 14)]]


@pytest.mark.parametrize("word", [P - 1, 0], ids=["all_p_minus_1", "all_0"])
@pytest.mark.parametrize("shapes", SHAPES, ids=str)
def test_merkle_commit_constant_matrices(gpu, oracle, shapes, word):
    mats = [np.full((w, 1 << lh), word, np.uint32) for w, lh in shapes]
    want = oracle.merkle_commit(mats)
    ts = [dev(m) for m in mats]
    for t in ts:
        gpu.to_internal(t)
    mx = max(lh for _, lh in shapes)
    dg = filled(((2 << mx) - 1) * 8)
    gpu.merkle_commit([(t, w, lh) for t, (w, lh) in zip(ts, shapes)], dg)
    gpu.from_internal(dg)
    gpu.sync()
    got = host(dg).reshape(-1, 8)
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, f"tree {shapes} of {word}: {bad.size} of {got.shape[0]} digests differ, first at {int(bad[0])}"
