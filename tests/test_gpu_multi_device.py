"""One handle, several device members ("devices": [d0, d1, ...]): shard i of an execution is proven on member i mod G behind
the same calls, and proof bytes, verifying key and container are those of the one-device, one-lane prover.  A device index
may repeat, so every case runs on a one-GPU machine as [0, 0] / [0, 0, 0]; the distinct-device cases ([0, 1], [0, 1, 2, 3])
skip with the device count in the reason where the machine has fewer GPUs."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import guests

pytestmark = pytest.mark.gpu

Q, POW = 8, 4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dvt_circuits_amd", "dvt_prover_host")


@pytest.fixture(scope="module")
def gpu():
    import torch

    assert torch.cuda.is_available()
    yield


def _cfg(log_shard, extra=""):
    return '{"fri_queries": %d, "pow_bits": %d, "log_shard_size": %d%s}' % (Q, POW, log_shard, extra)


def _single(log_shard, extra=""):
    """the reference of every comparison: one device, one lane"""
    from dvt_circuits_amd import capi

    return capi.Prover(_cfg(log_shard, ', "lanes": 1' + extra))


def _multi(devices, log_shard, extra=""):
    from dvt_circuits_amd import capi

    p = capi.Prover(_cfg(log_shard, ', "devices": %s%s' % (json.dumps(list(devices)), extra)))
    assert p.device_count() == len(devices)
    assert [p.device(m) for m in range(len(devices))] == list(devices) and p.device(len(devices)) == -1
    return p


def _need(devices):
    import torch

    have = torch.cuda.device_count()
    if max(devices) >= have:
        pytest.skip("devices %s need %d GPUs, torch.cuda.device_count() is %d" % (list(devices), max(devices) + 1, have))


def _per_shard(p, pk, vk, stdin, first=0, stride=1, ch=None):
    """the bench's loop: prepare -> commit_shard -> challenges -> prove_shard for each held shard"""
    from dvt_circuits_amd import capi

    job, _ = p.prepare(pk, stdin, first=first, stride=stride)
    n = p.job_shards(job)
    mine = list(range(first, n, stride))
    headers = {i: p.commit_shard(pk, job, i) for i in mine}
    if ch is None:
        assert stride == 1
        ch = capi.rv32_challenges(vk, [headers[i] for i in range(n)])
    proofs = [p.prove_shard(pk, job, i, ch) for i in mine]
    return job, headers, ch, proofs


def _three_ways(p, elf, stdin):
    """(container of the per-shard loop, prove_job container, prove_core container, vk); checks the placement of a full job"""
    G = p.device_count()
    pk, vk = p.setup(elf)
    job, _, _, proofs = _per_shard(p, pk, vk, stdin)
    assert [p.job_shard_member(job, i) for i in range(len(proofs))] == [i % G for i in range(len(proofs))]
    assert p.job_shard_member(job, len(proofs)) == -1
    loop = p.assemble(job, proofs)
    p.job_free(job)
    job, _ = p.prepare(pk, stdin)
    whole = p.prove_job(pk, job)
    again = p.prove_job(pk, job)          # the phase-1 results are consumed: every member commits its shards again
    assert again == whole
    p.job_free(job)
    core, _ = p.prove_core(pk, stdin)
    p.pk_free(pk)
    p.close()
    return loop, whole, core, vk


_REF = {}


def _ref_bignum(keep):
    if keep not in _REF:
        elf, want = guests.bignum(1, limbs=12)
        _REF[keep] = _three_ways(_single(10, ', "keep_phase1": %d' % keep), elf, ())
    return _REF[keep]


def _bytes_case(devices, keep):
    from dvt_circuits_amd import capi

    elf, want = guests.bignum(1, limbs=12)
    ref = _ref_bignum(keep)
    assert ref[0] == ref[1] == ref[2]
    ok, ec, pv, why = capi.verify(ref[3], ref[0], Q, POW)
    assert ok and ec == 0 and pv == want, why
    assert len(capi.split_container(ref[0])[2]) == 13
    got = _three_ways(_multi(devices, 10, ', "keep_phase1": %d' % keep), elf, ())
    assert got[3] == ref[3], "verifying key differs from the one-device key"
    for k in range(3):
        assert got[k] == ref[0], "devices %s, way %d: bytes differ from the one-device proof" % (list(devices), k)


@pytest.mark.parametrize("keep", [1, 0])
@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_members_on_one_gpu_reproduce_the_one_device_bytes(gpu, devices, keep):
    """13 shards by the per-shard loop, prove_job (twice) and prove_core on two and three members of GPU 0"""
    _bytes_case(devices, keep)


@pytest.mark.parametrize("devices", [(0, 1), (0, 1, 2, 3)])
def test_members_on_distinct_gpus_reproduce_the_one_device_bytes(gpu, devices):
    _need(devices)
    for keep in (1, 0):
        _bytes_case(devices, keep)


def _precompile_guest():
    from dvt_circuits_amd import capi

    with open(os.path.join(ROOT, "tests", "golden", "finalization_example.json"), "rb") as f:
        buf = capi.stdin_from_json("finalization", f.read())
    elf = guests.dkg_like("finalization", 1, 1, 1, sha_precompiles=True, curve_precompiles=True)
    want = guests.dkg_like_expected(buf, "finalization", 1, 1, 1, curve_precompiles=True)
    return elf, [buf], want


@pytest.mark.parametrize("keep", [1, 0])
def test_members_with_sha_and_curve_precompile_chips(gpu, keep):
    """shards with the short and wide precompile tables on two members (default lanes: two each)"""
    from dvt_circuits_amd import capi

    elf, stdin, want = _precompile_guest()
    extra = ', "keep_phase1": %d' % keep
    ref = _three_ways(_single(12, extra), elf, stdin)
    got = _three_ways(_multi((0, 0), 12, extra), elf, stdin)
    assert ref[0] == ref[1] == ref[2]
    assert got == ref
    ok, ec, pv, why = capi.verify(ref[3], ref[0], Q, POW)
    assert ok and ec == 0 and pv == want, why


def _partial_case(devices):
    G = len(devices)
    elf, _ = guests.bignum(1, limbs=12)
    p1 = _single(10)
    pk1, vk = p1.setup(elf)
    job, headers, ch, ref = _per_shard(p1, pk1, vk, ())
    n = p1.job_shards(job)
    assert [p1.job_shard_member(job, i) for i in range(n)] == [0] * n and p1.job_shard_member(job, n) == -1
    p1.job_free(job)
    p2 = _multi(devices, 10)
    pk2, vk2 = p2.setup(elf)
    assert vk2 == vk
    job, part_headers, _, got = _per_shard(p2, pk2, vk2, (), first=1, stride=2, ch=ch)
    held = list(range(1, n, 2))
    assert [p2.job_shard_member(job, i) for i in held] == [k % G for k in range(len(held))]
    for i in list(range(0, n, 2)) + [n, n + 1]:
        assert p2.job_shard_member(job, i) == -1
    for i in part_headers:
        assert np.array_equal(part_headers[i], headers[i])
    assert got == [ref[i] for i in held]
    p2.job_free(job)
    for p, pk in ((p1, pk1), (p2, pk2)):
        p.pk_free(pk)
        p.close()


@pytest.mark.parametrize("devices", [(0, 0), (0, 0, 0)])
def test_placement_on_a_partial_job(gpu, devices):
    """prepare(first=1, stride=2): the k-th held shard is on member k mod G, a shard not held on none, and the held shards'
    proofs under the full job's challenges equal the one-device ones"""
    _partial_case(devices)


@pytest.mark.parametrize("devices", [(0, 1), (0, 1, 2, 3)])
def test_placement_on_a_partial_job_distinct_gpus(gpu, devices):
    _need(devices)
    _partial_case(devices)


def test_early_exit_and_changed_challenges_on_two_members(gpu):
    """claim one shard and free the job (no hang; the next job's bytes still match), and a prove_shard with other challenges
    in between gives what one device gives for those challenges"""
    elf, _ = guests.bignum(1, limbs=12)
    p1 = _single(10)
    pk1, vk = p1.setup(elf)
    job, _, ch, ref = _per_shard(p1, pk1, vk, ())
    p1.job_free(job)
    other = np.array(ch, dtype=np.uint32).copy()
    other[0] = (int(other[0]) + 1) % 0x78000001
    job, _ = p1.prepare(pk1, ())
    ref_other = p1.prove_shard(pk1, job, 3, other)
    p1.job_free(job)

    p2 = _multi((0, 0), 10)
    pk2, _ = p2.setup(elf)
    job, _ = p2.prepare(pk2, ())
    assert p2.prove_shard(pk2, job, 0, ch) == ref[0]
    p2.job_free(job)
    job, _, _, got = _per_shard(p2, pk2, vk, ())
    assert got == ref
    p2.job_free(job)
    job, _ = p2.prepare(pk2, ())
    assert p2.prove_shard(pk2, job, 2, ch) == ref[2]
    assert p2.prove_shard(pk2, job, 3, other) == ref_other
    assert p2.prove_shard(pk2, job, 4, ch) == ref[4]
    p2.sync()
    p2.job_free(job)
    for p, pk in ((p1, pk1), (p2, pk2)):
        p.pk_free(pk)
        p.close()


def _late(kind, loops=700):
    """~2 * loops cycles of counting, then a misaligned load ("trap") or HALT(3) ("exit"): at log_shard_size 10 the failure
    lies in the second shard, which a two-member handle holds on member 1"""
    a = guests.Asm()
    a.li("s2", 0)
    a.li("s3", loops)
    a.label("loop")
    a.addi("s2", "s2", 1)
    a.bltu("s2", "s3", "loop")
    if kind == "trap":
        a.li("a3", 0x1000)
        a.lw("a4", "a3", 1)
        a.halt(0)
    else:
        a.halt(3)
    return a.elf()


def _errors_case(devices):
    from dvt_circuits_amd import capi

    for kind in ("trap", "exit"):      # the failure is in the second of two shards
        rc, rep, _, _ = capi.execute(_late(kind))
        assert rc == capi.DVT_ERR_GUEST and 1024 < rep["cycles"] <= 2048
    good, _ = guests.bignum(1, limbs=12)
    p1 = _single(10)
    pk1, vk = p1.setup(good)
    want, _ = p1.prove_core(pk1, ())
    p2 = _multi(devices, 10)
    for elf in (guests.exit_with(1), guests.traps(), _late("trap"), _late("exit")):     # member 0, member 0, member 1, member 1
        codes = []
        for p in (p1, p2):
            pk, _ = p.setup(elf)
            with pytest.raises(capi.DvtError) as e:
                p.prove_core(pk, ())
            codes.append(e.value.code)
            with pytest.raises(capi.DvtError) as e:
                p.prepare(pk, ())
            codes.append(e.value.code)
            p.pk_free(pk)
        assert codes == [capi.DVT_ERR_GUEST] * 4
        # the handle stays usable
        pk2, vk2 = p2.setup(good)
        assert vk2 == vk
        assert p2.prove_core(pk2, ())[0] == want
        p2.pk_free(pk2)
    p1.pk_free(pk1)
    p1.close()
    p2.close()


def test_guest_failures_on_two_members(gpu):
    """a guest that halts non-zero and one that traps, in a shard of member 0 and in a shard of member 1: DVT_ERR_GUEST as on
    one device, and a good prove_core on the same handle afterwards gives the one-device bytes"""
    _errors_case((0, 0))


def test_guest_failures_on_distinct_gpus(gpu):
    _need((0, 1))
    _errors_case((0, 1))


def test_device_list_config(gpu):
    import torch

    from dvt_circuits_amd import capi

    n = torch.cuda.device_count()
    bad = ['"devices": []', '"devices": [%s]' % ", ".join(["0"] * 9), '"devices": [-1]', '"devices": [%d]' % n,
           '"device": 0, "devices": [0]', '"devices": [0, "a"]', '"devices": [0.5]', '"devices": 0']
    for extra in bad:
        with pytest.raises(capi.DvtError) as e:
            capi.Prover(_cfg(10, ", " + extra))
        assert e.value.code == capi.DVT_ERR_INPUT and "device" in e.value.msg, extra
    elf, _ = guests.bignum(1, limbs=12)
    out = []
    for cfg in (_cfg(10), _cfg(10, ', "devices": [0]'), _cfg(10, ', "devices": [0, 0, 0, 0, 0, 0, 0, 0], "lanes": 1')):
        p = capi.Prover(cfg)
        pk, vk = p.setup(elf)
        out.append((p.device_count(), p.prove_core(pk, ())[0], vk))
        p.pk_free(pk)
        p.close()
    assert [o[0] for o in out] == [1, 1, 8]
    assert out[0][1:] == out[1][1:] == out[2][1:]


_ENV_CHILD = """
import sys
from dvt_circuits_amd import capi
p = capi.Prover('{"device": 0}')
print("members", p.device_count(), p.device(0), p.device(1))
p.close()
try:
    capi.Prover('{"device": 0, "devices": [0]}')
except capi.DvtError as e:
    print("both", e.code)
p = capi.Prover('{"devices": [0]}')
print("key wins", p.device_count())
"""


def test_device_list_from_the_environment(gpu):
    """DVT_DEVICES is read when the handle is made, so it is set in the environment of a child process: with a cfg that has
    only "device" it is the list; the cfg key "devices" goes before it; a bad list is refused"""
    env = dict(os.environ, DVT_DEVICES="0,0", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _ENV_CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split("\n")[:3] == ["members 2 0 0", "both 2", "key wins 1"]
    for bad in ("0,,0", "0,x", "-1", "0," * 8 + "0"):
        env = dict(os.environ, DVT_DEVICES=bad, PYTHONPATH=ROOT)
        r = subprocess.run([sys.executable, "-c", "from dvt_circuits_amd import capi\ntry:\n    capi.Prover('{}')\nexcept capi.DvtError as e:\n    print('refused', e.code)"],
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and r.stdout.strip() == "refused 2", (bad, r.stdout, r.stderr)


def test_a_two_member_handle_next_to_a_default_handle(gpu):
    """two host threads, one with a [0, 0] handle and one with a default handle, prove at the same time: both get the
    one-device bytes"""
    from dvt_circuits_amd import capi

    elf, _ = guests.bignum(1, limbs=12)
    p1 = _single(10)
    pk1, vk = p1.setup(elf)
    want, _ = p1.prove_core(pk1, ())
    p1.pk_free(pk1)
    p1.close()
    handles = [_multi((0, 0), 10), capi.Prover(_cfg(10))]
    got, errs = [[], []], []

    def run(k):
        try:
            h = handles[k]
            hpk, hvk = h.setup(elf)
            assert hvk == vk
            for rep in range(3):
                got[k].append(h.prove_core(hpk, ())[0])
            h.pk_free(hpk)
        except Exception as e:                                      # noqa: BLE001 - reported by the assert below
            errs.append(repr(e))

    th = [threading.Thread(target=run, args=(k,)) for k in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for h in handles:
        h.close()
    assert not errs, errs
    assert got == [[want] * 3, [want] * 3]


def test_key_or_job_of_a_handle_with_other_devices_is_refused(gpu):
    """a job prepared on [0, 0] given to a one-device handle (with that handle's own key), and the one-device key given to
    the [0, 0] handle with its job: every entry point that takes a key and a job answers DVT_ERR_INPUT; the [0, 0] handle
    then proves its job to the one-device bytes"""
    from dvt_circuits_amd import capi

    elf, _ = guests.bignum(1, limbs=12)
    p1 = _single(10)
    pk1, vk = p1.setup(elf)
    want, _ = p1.prove_core(pk1, ())
    p2 = _multi((0, 0), 10)
    pk2, vk2 = p2.setup(elf)
    assert vk2 == vk
    job, _ = p2.prepare(pk2, ())
    ch = np.arange(1, 9, dtype=np.uint32)
    for p in (p1, p2):                       # the key is p1's both times, the job p2's
        for call in (lambda: p.prove_job(pk1, job), lambda: p.check_job(pk1, job), lambda: p.commit_shard(pk1, job, 0),
                     lambda: p.prove_shard(pk1, job, 0, ch), lambda: p.debug_device_traces(pk1, job, 0)):
            with pytest.raises(capi.DvtError) as e:
                call()
            assert e.value.code == capi.DVT_ERR_INPUT and "other devices" in e.value.msg
    assert p2.prove_job(pk2, job) == want
    p2.job_free(job)
    for p, pk in ((p1, pk1), (p2, pk2)):
        p.pk_free(pk)
        p.close()


def test_cli_prove_on_two_members_then_verify(tmp_path):
    """`dvt_prover_host prove --devices 0,0` writes the proof the one-device CLI writes, and `verify` accepts it; a bad list is
    the library's DVT_ERR_INPUT, exit code 1"""
    import shutil

    (tmp_path / "finalization.elf").write_bytes(guests.hint_sum())
    inp = tmp_path / "in.json"
    shutil.copy(os.path.join(ROOT, "tests", "golden", "finalization_example.json"), inp)
    env = dict(os.environ, DVT_ELF_DIR=str(tmp_path))
    env.pop("DVT_DEVICES", None)
    one, two = str(tmp_path / "one.bin"), str(tmp_path / "two.bin")
    r = subprocess.run([CLI, "prove", "--type", "finalization", "-i", str(inp), "-o", one], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([CLI, "prove", "--type", "finalization", "-i", str(inp), "-o", two, "--devices", "0,0"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and f"Proof saved to: {two}" in r.stdout, r.stderr
    assert open(one, "rb").read() == open(two, "rb").read()
    r = subprocess.run([CLI, "verify", "--type", "finalization", "-i", two], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Proof verified" in r.stdout, r.stderr
    r = subprocess.run([CLI, "prove", "--type", "finalization", "-i", str(inp), "-o", str(tmp_path / "no.bin"), "--devices=0,x"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "devices" in r.stderr and not (tmp_path / "no.bin").exists()
