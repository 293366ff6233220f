"""stark_ntt_batch_dev / stark_lde_batch_dev without a device: the two symbols in the header, the ctypes table and the Rust declarations, and the
rule that cuts a batch into passes (csrc/ntt_batch_plan.hpp, through libstark_mlwe_hostcheck.so) against a plain-Python restatement.  CPU only."""
import ctypes as C
import os
import re

import numpy as np

import hostcheck_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"stark_ntt_batch_dev": 7, "stark_lde_batch_dev": 8}


def test_batch_symbols_in_header_ctypes_table_and_rust_declarations():
    from stark_mlwe_amd._abi import SIGNATURES
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stark_mlwe.h")).read(), flags=re.S)
    ffi = open(os.path.join(ROOT, "rust", "stark-mlwe-hip", "src", "ffi.rs")).read()
    for name, arity in ARITY.items():
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, "%s is not declared in include/stark_mlwe.h" % name
        assert len(m.group(1).split(",")) == arity, name
        assert name in SIGNATURES and len(SIGNATURES[name][1]) == arity and SIGNATURES[name][0] is C.c_int32, name
        r = re.search(r"pub fn %s\(([^)]*)\) -> i32;" % name, ffi)
        assert r and len(r.group(1).split(",")) == arity, name
    lib_rs = open(os.path.join(ROOT, "rust", "stark-mlwe-hip", "src", "lib.rs")).read()
    assert "stark_lde_batch_dev(" in lib_rs and "stark_ntt_batch_dev(" in lib_rs, "no wrapper in lib.rs"
    from stark_mlwe_amd.api import Context
    assert callable(Context.ntt_batch_dev) and callable(Context.lde_batch_dev)


def passes_ref(batch, log_out, limit):
    """columns per pass: as many whole columns as fit under the limit, at least one, in the caller's order"""
    per = max(limit // (1 << log_out), 1)
    out = []
    while batch > 0:
        out.append(min(per, batch)); batch -= out[-1]
    return out


def passes_lib(lib, batch, log_out, limit):
    buf = (C.c_size_t * 16)()
    lib.hc_ntt_batch_passes.restype = C.c_size_t
    k = lib.hc_ntt_batch_passes(C.c_size_t(batch), C.c_int(log_out), C.c_size_t(limit), buf, C.c_size_t(16))
    assert k <= 16
    return [int(buf[i]) for i in range(k)]


def test_pass_cutting_agrees_with_a_plain_restatement_and_keeps_its_promises():
    lib = C.CDLL(hostcheck_lib.PATH)
    for batch in range(0, 10):
        for log_out in range(0, 27):
            for log_limit in range(10, 27):
                for limit in {1 << log_limit, (1 << log_limit) + 1, 3 << (log_limit - 1)}:
                    got = passes_lib(lib, batch, log_out, limit)
                    assert got == passes_ref(batch, log_out, limit), (batch, log_out, limit, got)
                    assert sum(got) == batch and all(p >= 1 for p in got), (batch, log_out, limit, got)             # every column once, in order: passes are consecutive runs
                    assert all(p == 1 or (p << log_out) <= limit for p in got), (batch, log_out, limit, got)       # over the limit only as a pass of one column
                    assert all(p == got[0] for p in got[:-1]) and (not got or got[-1] <= got[0]), (batch, log_out, limit, got)
    assert passes_lib(lib, 5, 11, 2 << 11) == [2, 2, 1]
    assert passes_lib(lib, 64, 11, 1 << 24) == [64] and passes_lib(lib, 4, 23, 1 << 24) == [2, 2] and passes_lib(lib, 3, 25, 1 << 24) == [1, 1, 1]


def test_output_ranges_overlap_check():
    lib = C.CDLL(hostcheck_lib.PATH)

    def overlap(starts, nbytes):
        a = np.array(starts, np.uint64)
        return lib.hc_ntt_batch_ranges_overlap(a.ctypes.data_as(C.c_void_p), C.c_size_t(len(starts)), C.c_size_t(nbytes))
    assert overlap([], 32) == 0 and overlap([4096], 32) == 0
    assert overlap([4096, 4096 + 64, 4096 + 32], 32) == 0                 # adjacent, out of order
    assert overlap([4096, 8192, 4096], 32) == 1                           # the same range twice
    assert overlap([4096, 4096 + 31], 32) == 1 and overlap([4096 + 31, 4096], 32) == 1
    assert overlap([(1 << 63) + 4096, 4096, (1 << 63) + 4096 + 1024], 1024) == 0
