"""The lane-group SpMM planner on the host, shared by the CPU and the GPU tests: tests/hostcheck/plancheck.cpp is the
g++ build of neurec_amd/csrc/spmm_blocked_plan.h, the very header nrhip_spmm_blocked_plan_create calls.  build() runs it
with every option explicit and hands out the schedule's arrays; same_plan() compares a device plan buffer, copied to the
host, with such a host plan byte for byte — so "the kernel walked the plan the test restated" is an assertion and not an
assumption about two compilers' std::sort."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = 2
MAX_LDS = 160 * 1024

SCALARS = ["n_rows", "nnz", "n_wg", "n_phases", "nnz_cap", "ent_cap", "colmask_ok", "wanted_ok", "w_ent_cap", "w_nnz_cap",
           "w_bitmap_words", "ww_ok", "ww_ent_cap", "ww_lds_slots", "ww_segments", "seg", "r_max", "p_max", "waves",
           "split_row"]
ARRAYS = {"wg_row0": np.int32, "wg_nrows": np.int32, "row_of": np.int32, "pk_src": np.uint32, "pk_dst": np.uint32,
          "ent_off": np.int32, "cmb_off": np.int32, "ent": np.int32, "cmb": np.int32, "wg_nnz": np.uint32,
          "w_ent": np.int32, "w_cmb": np.int32, "w_ent_off": np.int32, "w_cmb_off": np.int32,
          "ww_off": np.int32, "ww_choff": np.int32, "ww_lcoff": np.int32, "ww_ent": np.int32, "ww_gch": np.int32,
          "ww_hub": np.int32, "ww_lcmb": np.int32}
INT4 = ("ent", "cmb", "w_ent", "w_cmb", "ww_ent", "ww_hub", "ww_lcmb")
# plan_sections' order (spmm_blocked_plan.h; test_spmm_plan_cpu.check_layout pins every section's size in this order);
# None: a section the device fills (the packed pairs, the partial sums and counters of the wave-cooperative hop)
SECTIONS = ["ent", "cmb", "wg_row0", "wg_nrows", "row_of", "pk_src", "pk_dst", None, None, "ent_off", "cmb_off",
            "wg_nnz", "w_ent", "w_cmb", "w_ent_off", "w_cmb_off"]
SECTIONS_WW = ["ww_off", "ww_choff", "ww_ent", "ww_gch", "ww_hub", "ww_lcoff", "ww_lcmb", None, None]

_LIB = []


def load_plancheck():
    """libplancheck.so, rebuilt when its source or the planner header is newer"""
    if _LIB:
        return _LIB[0]
    d = os.path.join(ROOT, "tests", "hostcheck")
    so, src = os.path.join(d, "libplancheck.so"), os.path.join(d, "plancheck.cpp")
    hdr = os.path.join(ROOT, "neurec_amd", "csrc", "spmm_blocked_plan.h")
    if (not os.path.isfile(so)) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall",
                               "-I", os.path.join(ROOT, "neurec_amd", "csrc"), "-o", so, src])
    lib = C.CDLL(so)
    lib.pc_plan_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int, C.c_int64] + [C.c_int] * 8 + \
                                  [C.c_char_p, C.c_int, C.POINTER(C.c_void_p)]
    lib.pc_plan_destroy.argtypes = [C.c_void_p]
    lib.pc_plan_destroy.restype = None
    lib.pc_scalar.argtypes = [C.c_void_p, C.c_char_p]
    lib.pc_scalar.restype = C.c_int64
    lib.pc_array.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    lib.pc_sections.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int64)]
    lib.pc_plan_bytes.argtypes = [C.c_int64, C.c_int64]
    lib.pc_plan_bytes.restype = C.c_int64
    _LIB.append(lib)
    return lib


class Refused(Exception):
    def __init__(self, code, msg):
        Exception.__init__(self, msg)
        self.code = code


def build(lib, A, d, n_wg, split_row=0, block_bytes=0, waves=0, seg=0, r_max=0, p_max=0, masked_fast=1, wanted_wave=1,
          wanted_nnz_cap=0):
    """run the planner; returns a dict of its scalars, arrays (copies; int4 arrays as [n, 4]) and section layout"""
    indptr = np.ascontiguousarray(A.indptr, np.int64)
    indices = np.ascontiguousarray(A.indices, np.int32)
    err = C.create_string_buffer(512)
    h = C.c_void_p(0)
    rc = lib.pc_plan_create(indptr.ctypes.data, indices.ctypes.data, len(indptr) - 1, split_row, d, block_bytes, n_wg,
                            waves, seg, r_max, p_max, masked_fast, wanted_wave, wanted_nnz_cap, err, 512, C.byref(h))
    if rc != 0:
        raise Refused(rc, err.value.decode())
    try:
        P = {k: int(lib.pc_scalar(h, k.encode())) for k in SCALARS}
        for name, dt in ARRAYS.items():
            data, nbytes = C.c_void_p(0), C.c_int64(0)
            assert lib.pc_array(h, name.encode(), C.byref(data), C.byref(nbytes)) == 1, name
            a = np.frombuffer(C.string_at(data.value, nbytes.value), dtype=dt).copy() if nbytes.value else np.zeros(0, dt)
            P[name] = a.reshape(-1, 4) if name in INT4 else a
        off, size, used = np.zeros(64, np.int64), np.zeros(64, np.int64), C.c_int64(0)
        n = lib.pc_sections(h, off.ctypes.data, size.ctypes.data, 64, C.byref(used))
        P["sec_off"], P["sec_size"], P["used"] = off[:n], size[:n], used.value
    finally:
        lib.pc_plan_destroy(h)
    P["d"], P["block_bytes"] = d, block_bytes
    return P


def same_plan(buf, info, P):
    """buf: the device plan buffer copied to the host (uint8); info: nrhip_spmm_blocked_plan_info's four numbers
    (workgroups, phases, entries, combine records).  Asserts that every array the kernels walk holds the host plan's
    bytes at the offset pc_sections reports; returns the number of arrays compared."""
    assert tuple(int(x) for x in info) == (P["n_wg"], P["n_phases"], len(P["ent"]), len(P["cmb"])), (info, P["n_wg"])
    names = SECTIONS + (SECTIONS_WW if P["ww_ok"] else [])
    assert len(names) == len(P["sec_off"]), (len(names), len(P["sec_off"]))
    buf = np.asarray(buf).view(np.uint8).ravel()
    assert buf.size >= P["used"]
    n = 0
    for name, off in zip(names, P["sec_off"].tolist()):
        if name is None:
            continue
        want = np.ascontiguousarray(P[name]).view(np.uint8).ravel()
        assert np.array_equal(buf[off:off + want.size], want), "device plan differs from the host plan in " + name
        n += 1
    return n
