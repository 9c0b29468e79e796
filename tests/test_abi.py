"""C-ABI library: loads, exports every symbol include/gnsship.h declares, host-only entry points
(code generators) agree with the reference fixtures, error paths return codes (CPU only)."""
import ctypes
import os

import numpy as np

from gnss_sim_receiver_amd import abi, codes

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def test_library_exports_every_declared_symbol(built):
    lib = abi.load()
    names = abi.declared_symbols()
    assert len(names) >= 35
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert lib.gnsship_abi_version() == abi.ABI_VERSION == 2
    # and every declared symbol has a ctypes signature in the binding
    assert set(names) <= set(abi._SIGNATURES), set(names) - set(abi._SIGNATURES)


def test_product_code_generators_match_reference(built):
    g = np.load(os.path.join(GOLD, "codes_ref.npz"))
    for k in range(32):
        assert (codes.gps_l1_ca_code_gen_float(k + 1) == g["gps"][k]).all()
    for k in range(63):
        assert (codes.beidou_b1i_code_gen_float(k + 1) == g["b1i"][k]).all()
    for key in g.files:
        if key.startswith("gps_sampled_"):
            fs, prn = map(int, key.split("_")[2:])
            c = codes.gps_l1_ca_code_gen_complex_sampled(prn, fs)
            assert (c.imag == g[key]).all() and (c.real == 0).all()
        if key.startswith("b1i_sampled_"):
            fs, prn = map(int, key.split("_")[2:])
            assert (codes.beidou_b1i_code_gen_complex_sampled(prn, fs).real == g[key]).all()


def test_code_generator_rejects_bad_prn(built):
    out = np.zeros(1023, np.float32)
    assert abi.load().gnsship_gps_l1_ca_code_gen_float(abi.fptr(out), 0, 0) == abi.E_INVAL
    assert abi.load().gnsship_gps_l1_ca_code_gen_float(abi.fptr(out), 211, 0) == abi.E_INVAL
    assert abi.load().gnsship_beidou_b1i_code_gen_float(abi.fptr(out), 64, 0) == abi.E_INVAL


def test_null_arguments_are_rejected_without_device(built):
    lib = abi.load()
    assert lib.gnsship_ctx_create(0, None) == abi.E_INVAL
    assert lib.gnsship_ctx_destroy(None) == abi.E_INVAL
    assert lib.gnsship_corr_destroy(None) == abi.E_INVAL
    assert lib.gnsship_batch_set_jobs(None, None, 0, 0) == abi.E_INVAL
    assert lib.gnsship_acq_run(None, None, 0, 0, 1, None, None) == abi.E_INVAL
    assert lib.gnsship_last_error(None) == b"null context"


def test_job_layout_matches_header(built):
    assert abi.JOB_DTYPE.itemsize == 80
    assert ctypes.sizeof(abi.AcqResult) == 32
    assert ctypes.sizeof(abi.AcqConf) == 64
    assert ctypes.sizeof(abi.AcqLayout) == 84
    assert ctypes.sizeof(abi.TrkPlan) == 64
