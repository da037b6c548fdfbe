"""CPU tests of the device verifier's ABI (include/dvt_prover.h, ABI 7): the new symbols exist, a NULL handle is an input
error, and the host verifier, whose shard check is now a host part plus a per-query part, still accepts the committed
fixtures and names the same reasons on tampered copies."""
import ctypes as C
import os
import struct

import numpy as np

from dvt_circuits_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, POW = 4, 4
P = 2013265921


def _load(name):
    blob = open(os.path.join(ROOT, "tests", "golden", f"proof_{name}.bin"), "rb").read()
    (n,) = struct.unpack_from("<I", blob)
    return blob[4:4 + n], blob[4 + n:]


def test_new_symbols_are_exported_and_the_abi_is_7():
    lib = capi.load()
    for name in ("dvt_prover_verify", "dvt_prover_machine_verify", "dvt_stage_sponge_rows", "dvt_stage_verify_paths"):
        assert hasattr(lib, name), name
    assert lib.dvt_abi_version() >= 7
    assert hasattr(capi.Prover, "verify") and hasattr(capi.Prover, "machine_verify")


def test_null_handle_is_an_input_error():
    lib = capi.load()
    vk, proof = _load("commit")
    why = C.c_char_p()
    ec, pv, n = C.c_int32(), capi.u8p(), C.c_size_t()
    rc = lib.dvt_prover_verify(None, vk, len(vk), proof, len(proof), Q, POW, C.byref(ec), C.byref(pv), C.byref(n), C.byref(why))
    assert rc == capi.DVT_ERR_INPUT and not pv
    if why.value is not None:
        lib.dvt_free(C.cast(why, C.c_void_p))
    why = C.c_char_p()
    rc = lib.dvt_prover_machine_verify(None, vk, len(vk), proof, len(proof), Q, POW, C.byref(why))
    assert rc == capi.DVT_ERR_INPUT
    if why.value is not None:
        lib.dvt_free(C.cast(why, C.c_void_p))
    assert lib.dvt_stage_sponge_rows(None, None, None, 0, None) == capi.DVT_ERR_INPUT
    assert lib.dvt_stage_verify_paths(None, None, 0, None) == capi.DVT_ERR_INPUT


def test_host_verifier_keeps_its_decisions_and_reasons():
    for name in ("commit", "curve"):
        vk, proof = _load(name)
        ok, ec, _, why = capi.verify(vk, proof, Q, POW)
        assert ok and ec == 0 and why == "", (name, why)
    vk, proof = _load("commit")
    words = np.frombuffer(proof, np.uint32)
    # (positions by what they hold in the commit fixture: a main-root word, a word of the last query's last FRI path,
    # the length word of the first shard)
    shard0 = 4 + (int(words[3]) + 3) // 4
    for pos, want in ((shard0 + 2, "shard 1: constraint check failed at zeta for chip"), (len(words) - 1, "shard 5: Merkle opening rejected (FRI layer)"),
                      (shard0, "container truncated")):
        w = words.copy()
        w[pos] = (int(w[pos]) + 1) % P if w[pos] < P else int(w[pos]) - 1
        ok, _, _, why = capi.verify(vk, w.tobytes(), Q, POW)
        assert not ok and why.startswith(want), (pos, why)
