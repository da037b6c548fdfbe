"""GPU parity tests (run with -m gpu on an MI355X) for the two kernel families every committed column goes through,
at the shapes where their launch code changes kernel: the coset LDE (K1, csrc/ntt.hip launch_coset_lde) and the
mixed-height Merkle commitment (K2 / K3, csrc/merkle.hip under Engine::commit_tree), word for word against the CPU
oracle.  Integer work: every comparison is exact.

The shapes are tied to these dispatch constants; whoever retunes one moves the shapes with it:
  MERKLE_TOP_LOG = 6    layers of at most 2^6 nodes go down to the root in the one launch of merkle_top_kernel
  MERKLE_COOP_LOG = 13  levels (and leaf segments) above 2^13 nodes run one node per thread, the others 16 lanes per node
  7000 and 9.0          launch_merkle_leaves: work_us = sum_segments 2^log_h * ceil(ncols / 8) / 7000,
                        chain_us = 9.0 * ceil(ncols / 8); a segment is "coop" iff log_h <= 13 and chain_us > work_us
                        (a segment = all the matrices of one height, concatenated)
  12                    launch_coset_lde: blocks of 2^12 points (log_n2 = min(log_n, 12)), strided passes of
                        2^log_n1 = 2^(log_n - 12) rows; at log_n >= 12 column pairs take lde_block2_kernel
  V4_L = 9              log_n1 = 9 (log_n = 21) is the one size of ntt_strided_v4_kernel"""
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


# The stage entry points run on the prover's stream (non-blocking, not ordered with torch's), torch on its own: every
# buffer torch writes or fills is complete before a stage reads or writes it (torch.cuda.synchronize) - a fill that
# lands late would wipe what the kernels wrote - and the stage's results are read after gpu.sync().  torch.empty
# launches nothing and needs no such care.
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


# ------------------------------------------------------------------------------------------------ Merkle trees
def tree_matrices(shapes, seed):
    """[width][2^log_height] seeded words in [0, P) per shape; row 0 all 0, the last row all P - 1"""
    rng = np.random.default_rng(seed)
    mats = []
    for w, lh in shapes:
        m = rng.integers(0, P, (w, 1 << lh), dtype=np.uint32)
        m[:, 0] = 0
        m[:, -1] = P - 1
        mats.append(m)
    return mats


def gpu_tree(gpu, mats, shapes):
    """every layer of the GPU's tree, canonical: [(2H - 1)][8].  The digest buffer starts as zeros, so that a node no
    kernel wrote shows as a difference and not as whatever the allocation held."""
    ts = [dev(m) for m in mats]
    for t in ts:
        gpu.to_internal(t)
    mx = max(lh for _, lh in shapes)
    dg = filled(((2 << mx) - 1) * 8)
    gpu.merkle_commit([(t, w, lh) for t, (w, lh) in zip(ts, shapes)], dg)
    gpu.from_internal(dg)
    gpu.sync()
    return host(dg).reshape(-1, 8)


def first_bad_node(got, want, log_h):
    """None, or a text naming the first differing layer (by its height) and node"""
    bad = np.nonzero((got != want).any(axis=1))[0]
    if bad.size == 0:
        return None
    at, off = int(bad[0]), 0
    for lh in range(log_h, -1, -1):
        if at < off + (1 << lh):
            return (f"{bad.size} of {got.shape[0]} digests differ, first in the layer of 2^{lh} nodes at node {at - off}: "
                    f"{got[at].tolist()} != {want[at].tolist()}")
        off += 1 << lh


def check_tree(gpu, oracle, shapes, seed):
    mats = tree_matrices(shapes, seed)
    want = oracle.merkle_commit(mats)
    got = gpu_tree(gpu, mats, shapes)
    assert got.shape == want.shape
    msg = first_bad_node(got, want, max(lh for _, lh in shapes))
    assert msg is None, f"tree {shapes}: {msg}"


# 2^14 rows are never coop (log_h > MERKLE_COOP_LOG): hash_row, one row per thread.  Widths 1 and 7 are one short block
# (the words beyond it are the zeros of the fresh state), 9 is a whole block and a last block of 1 word (the state words
# beyond it must keep the first permutation's output), 16 is two whole blocks, and in (5,14) + (6,14) the first 8-word
# block takes words of both matrices and the second is 3 words long.
@pytest.mark.parametrize("shapes", [[(1, 14)], [(7, 14)], [(9, 14)], [(16, 14)], [(5, 14), (6, 14)]], ids=str)
def test_merkle_row_per_thread_leaves_ragged_block(gpu, oracle, shapes):
    check_tree(gpu, oracle, shapes, 20)


# levels of more than 2^13 nodes: merkle_level_kernel<false> is level 14 of [(3,15)] and of no other level here;
# merkle_level_kernel<true> is levels 15 and 14 of the second tree, both injected (13 and below go to the coop kernel)
@pytest.mark.parametrize("shapes", [[(3, 15)], [(3, 16), (2, 15), (9, 14)]], ids=str)
def test_merkle_row_per_thread_levels(gpu, oracle, shapes):
    check_tree(gpu, oracle, shapes, 21)


# where the injected digests change hands: level 13 is the first that launch_merkle_level gives to the coop kernel; with a
# start layer of 2^9 the level launches inject at 7 and 6 and merkle_top_kernel at 5; with a start layer of 2^6 there is
# no level launch and the top kernel injects at 5; 2^7 alone is one level launch before the top kernel, 2^6 alone none.
@pytest.mark.parametrize("shapes", [[(2, 15), (5, 13)], [(2, 9), (3, 7), (3, 6), (3, 5)], [(2, 6), (3, 5)], [(2, 7)], [(2, 6)]], ids=str)
def test_merkle_injection_at_the_seams(gpu, oracle, shapes):
    check_tree(gpu, oracle, shapes, 22)


@pytest.mark.parametrize("shapes", [[(3, 15), (100, 6)], [(3, 15), (1245, 4)], [(2, 15), (200, 9), (1, 12), (30, 3)]], ids=str)
def test_merkle_mixed_leaf_launch(gpu, oracle, shapes):
    """Several segments in one leaf launch, given in an order that launch_merkle_leaves has to sort (widest first), with
    coop and row-per-thread segments side by side - the short, wide precompile table behind tall leaves.  With
    work_us = sum 2^log_h * ceil(w / 8) / 7000 and chain_us = 9 * ceil(w / 8), coop iff log_h <= 13 and chain_us > work_us:
      [(3,15),(100,6)]:   work_us = 32768/7000 + 64*13/7000 = 4.68 + 0.12 = 4.80.  (100,6): chain_us = 9*13 = 117 -> coop;
                          (3,15): log_h > 13 -> row per thread.  Launch order (100,6), (3,15): 4 coop blocks, then 128.
      [(3,15),(1245,4)]:  work_us = 4.68 + 16*156/7000 = 5.04.  (1245,4): chain_us = 9*156 = 1404 -> coop (one block);
                          (3,15) row per thread.
      [(2,15),(200,9),(1,12),(30,3)]: work_us = 4.68 + 512*25/7000 + 4096/7000 + 8*4/7000 = 4.68 + 1.83 + 0.59 + 0.005 = 7.10.
                          (200,9): 225 -> coop; (30,3): 36 -> coop; (1,12): 9 > 7.10 -> coop; (2,15) row per thread.
                          Launch order 200, 30, 2, 1: coop, coop, row per thread, coop."""
    check_tree(gpu, oracle, shapes, 23)


# The coop decision for a 2^13 segment beside 2^16 leaves (work_us, chain_us as above):
#   [(8,16),(8,13)]:  work_us = 65536*1/7000 + 8192*1/7000 = 9.36 + 1.17 = 10.53 >= chain_us = 9*1 = 9    -> row per thread
#   [(8,16),(24,13)]: work_us = 9.36 + 8192*3/7000 = 9.36 + 3.51 = 12.87 <  chain_us = 9*3 = 27           -> coop
@pytest.mark.parametrize("shapes", [[(8, 16), (8, 13)], [(8, 16), (24, 13)]], ids=str)
def test_merkle_coop_decision(gpu, oracle, shapes):
    check_tree(gpu, oracle, shapes, 24)


def test_merkle_every_level_injected(gpu, oracle):
    """17 segments in one leaf launch (the block0 search goes all the way), an injection at every level from 15 to 0:
    merkle_level_kernel<true> at 15 and 14, the coop level kernel from 13 to 6, merkle_top_kernel from 5 to 0.
    (work_us = (2^17 - 1) / 7000 = 18.7 > chain_us = 9: every segment is row per thread.)"""
    check_tree(gpu, oracle, [(1 + h % 3, h) for h in range(17)], 25)


def test_merkle_commit_refuses_zero_width_and_too_tall(gpu, oracle):
    """A width-0 matrix (Engine::commit_tree would skip it: as the tallest the leaf layer stays unwritten, lower down
    the oracle injects the sponge of the empty row and the GPU nothing) and a log_height of 24 are DVT_ERR_INPUT with
    a message; the handle stays usable."""
    import torch
    from dvt_circuits_amd import capi

    def refused(mats, dg):
        arr = (capi.DevMatrix * len(mats))(*[capi.DevMatrix(t.data_ptr(), w, lh) for t, w, lh in mats])
        assert dg.numel() >= gpu.lib.dvt_merkle_digest_words(arr, len(mats))
        rc = gpu.lib.dvt_stage_merkle_commit(gpu.h, arr, len(mats), dg.data_ptr())
        return rc, gpu.lib.dvt_last_error(gpu.h).decode()

    # buffers sized for what an unchecked call would read and write
    some = dev(np.zeros(3 << 5, np.uint32))
    dg = filled(((2 << 5) - 1) * 8)
    for mats in ([(some, 0, 5), (some, 3, 4)], [(some, 3, 5), (some, 0, 3)], [(some, 0, 0)]):
        rc, msg = refused(mats, dg)
        assert rc == capi.DVT_ERR_INPUT and "width 0" in msg, ([m[1:] for m in mats], rc, msg)
    tall = torch.empty(1 << 24, dtype=torch.int32, device="cuda")           # (never touched)
    dg_tall = torch.empty(((2 << 24) - 1) * 8, dtype=torch.int32, device="cuda")
    rc, msg = refused([(tall, 1, 24)], dg_tall)
    assert rc == capi.DVT_ERR_INPUT and "tree too tall" in msg, (rc, msg)
    del tall, dg_tall
    gpu.sync()
    assert (host(dg) == 0).all(), "a refused commit wrote digests"
    check_tree(gpu, oracle, [(3, 5), (2, 3)], 26)


# ------------------------------------------------------------------------------------------------ coset LDE
def lde_shift(log_n, shift_mode):
    return {0: 31, 1: 1, 2: pow(pow(31, (P - 1) >> (log_n + 1), P), -1, P)}[shift_mode]


def gpu_lde(gpu, m, log_n, shift_mode, scratch=None):
    """(output [width][2N] canonical, the input tensor as the call left it, still internal)"""
    width = m.shape[0]
    t_in = dev(m)
    t_out = filled(width << (log_n + 1))
    gpu.to_internal(t_in)
    gpu.coset_lde(t_in, t_out, width, log_n, shift_mode, scratch)
    gpu.from_internal(t_out)
    gpu.sync()
    return host(t_out).reshape(width, -1), t_in


def first_bad_word(got, want):
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    c, i = (int(x) for x in bad[0])
    return f"{bad.shape[0]} of {got.size} outputs differ, first in column {c} at index {i}: {int(got[c, i])} != {int(want[c, i])}"


# log_n 15, 17, 19, 20: strided passes of 2^3, 2^5, 2^7, 2^8 rows (tile 2^log_n1 x 2^(13 - log_n1), 2^4 columns at the
# least), none of them the V4 kernel's; width 3 = one column pair (lde_block2_kernel) + the odd last column
# (lde_block_kernel at an offset).  Width 1 skips the pair kernel, width 2 the single-column one; log_n 12 has no
# strided pass, 13 the smallest.
@pytest.mark.parametrize("log_n,width,shift_mode", [(15, 3, 0), (17, 3, 0), (19, 3, 0), (20, 3, 0), (15, 3, 2), (19, 3, 2), (17, 3, 1),
                                                    (12, 1, 0), (13, 1, 0), (15, 1, 0), (12, 2, 0)])
def test_coset_lde_strided_sizes_and_widths(gpu, oracle, log_n, width, shift_mode):
    rng = np.random.default_rng(300 + 10 * log_n + width)
    m = rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    want = oracle.coset_lde(m, 1, lde_shift(log_n, shift_mode))
    got, _ = gpu_lde(gpu, m, log_n, shift_mode)
    msg = first_bad_word(got, want)
    assert msg is None, f"log_n {log_n}, width {width}, shift_mode {shift_mode}: {msg}"


@pytest.mark.parametrize("log_n", [10, 13, 15])
def test_coset_lde_with_scratch_keeps_input(gpu, oracle, log_n):
    """With d_scratch given (as Engine::setup and the trace commitment give it) the first strided pass writes there:
    the output is the NULL-scratch output and d_in still holds the input.  include/dvt_prover.h leaves the contents of
    d_scratch after the call unspecified at every size - at log_n <= 12 no kernel is given it, and nothing may rely on
    that.  So the log_n = 10 case asserts nothing about the scratch itself: it only shows that a call with a scratch
    present gives the right output and keeps d_in, as the call without one does."""
    width = 3
    rng = np.random.default_rng(400 + log_n)
    m = rng.integers(0, P, (width, 1 << log_n), dtype=np.uint32)
    want = oracle.coset_lde(m, 1, 31)
    plain, _ = gpu_lde(gpu, m, log_n, 0)
    scratch = filled(width << log_n, 0x5A5A5A5A)
    got, t_in = gpu_lde(gpu, m, log_n, 0, scratch)
    msg = first_bad_word(got, want)
    assert msg is None, f"log_n {log_n} with scratch: {msg}"
    msg = first_bad_word(got, plain)
    assert msg is None, f"log_n {log_n}, scratch against NULL scratch: {msg}"
    gpu.from_internal(t_in)
    gpu.sync()
    msg = first_bad_word(host(t_in).reshape(width, -1), m)
    assert msg is None, f"log_n {log_n}: d_in did not survive: {msg}"


@pytest.mark.parametrize("log_n", [9, 13, 15])
@pytest.mark.parametrize("shift_mode", [0, 2])
def test_coset_lde_extreme_columns(gpu, oracle, log_n, shift_mode):
    """The butterflies state |a - b| < 2^35 and |v| < 2^33 for their FP64 products; columns whose transforms pile the
    largest word up (constant, alternating, half, a single P - 1 at the end) instead of uniform random words."""
    n = 1 << log_n
    m = np.zeros((4, n), np.uint32)
    m[0] = P - 1
    m[1, 1::2] = P - 1
    m[2, : n // 2] = P - 1
    m[3, n - 1] = P - 1
    want = oracle.coset_lde(m, 1, lde_shift(log_n, shift_mode))
    got, _ = gpu_lde(gpu, m, log_n, shift_mode)
    msg = first_bad_word(got, want)
    assert msg is None, f"log_n {log_n}, shift_mode {shift_mode}: {msg}"
