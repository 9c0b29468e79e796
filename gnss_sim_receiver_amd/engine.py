"""Thin Python handles over the C ABI, used by the tests, the bench and the smoke entry point.

The classes mirror the reference's engine objects one-to-one:

* :class:`MultiCorrelatorRealCodes` — ``Cpu_Multicorrelator_Real_Codes``
  (src/algorithms/tracking/libs/cpu_multicorrelator_real_codes.h:37-61): ``init``,
  ``set_local_code_and_taps``, ``set_input_output_vectors``,
  ``Carrier_wipeoff_multicorrelator_resampler``, ``free`` with the same argument meaning.
* :class:`CorrelatorBatch` — many (channel, epoch) correlations in one device launch.
* :class:`PcpsAcquisition` — ``pcps_acquisition::set_local_code`` / ``init`` / ``acquisition_core``.

All compute runs in ``libgnsship.so`` (HIP, gfx950).  These wrappers only move arguments.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import numpy as np

from . import abi
from .abi import FMT_CF32, FMT_CI8, FMT_CI16, JOB_DTYPE, MAX_TAPS, check, fptr

_FMT_OF_DTYPE = {np.dtype(np.complex64): FMT_CF32, np.dtype(np.int16): FMT_CI16, np.dtype(np.int8): FMT_CI8}
_FMT_BYTES = {FMT_CF32: 8, FMT_CI16: 4, FMT_CI8: 2}


def sample_format(x: np.ndarray) -> int:
    """complex64 → CF32 (gr_complex); int16 [..., 2] interleaved → CI16; int8 interleaved → CI8."""
    try:
        return _FMT_OF_DTYPE[x.dtype]
    except KeyError as e:
        raise TypeError(f"unsupported IF sample dtype {x.dtype}") from e


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = abi.load().gnsship_device_count(ctypes.byref(n))
    return n.value if rc == abi.OK else 0


class Context:
    """One HIP device, one stream, one code bank."""

    def __init__(self, device: int = 0):
        self.lib = abi.load()
        h = ctypes.c_void_p()
        check(self.lib.gnsship_ctx_create(device, ctypes.byref(h)), f"gnsship_ctx_create(device={device})")
        self.h = h
        self.device = device

    def close(self):
        if self.h:
            self.lib.gnsship_ctx_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self.lib.gnsship_ctx_sync(self.h), "gnsship_ctx_sync", self.h)

    def stream(self) -> int:
        s = ctypes.c_void_p()
        check(self.lib.gnsship_ctx_stream(self.h, ctypes.byref(s)), "gnsship_ctx_stream", self.h)
        return s.value or 0

    def event_record(self, slot: int):
        check(self.lib.gnsship_ctx_event_record(self.h, slot), "gnsship_ctx_event_record", self.h)

    def event_elapsed_ms(self, a: int, b: int) -> float:
        ms = ctypes.c_float()
        check(self.lib.gnsship_ctx_event_elapsed_ms(self.h, a, b, ctypes.byref(ms)), "gnsship_ctx_event_elapsed_ms", self.h)
        return ms.value

    def set_code(self, code_id: int, code: np.ndarray):
        code = np.ascontiguousarray(code, np.float32)
        check(self.lib.gnsship_code_set(self.h, code_id, fptr(code), len(code)), "gnsship_code_set", self.h)

    def upload(self, host: np.ndarray) -> "DeviceBuffer":
        buf = DeviceBuffer(self, host.nbytes)
        buf.upload(host)
        return buf


class DeviceBuffer:
    """An HBM allocation owned by a context (the IF sample buffer lives in one)."""

    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        p = ctypes.c_void_p()
        check(ctx.lib.gnsship_dev_alloc(ctx.h, nbytes, ctypes.byref(p)), f"gnsship_dev_alloc({nbytes})", ctx.h)
        self.ptr = p.value
        self.nbytes = nbytes
        self.owned = True

    @classmethod
    def wrap(cls, ctx: Context, ptr: int, nbytes: int) -> "DeviceBuffer":
        """A non-owning view of device memory allocated elsewhere (e.g. a torch tensor's storage)."""
        b = cls.__new__(cls)
        b.ctx, b.ptr, b.nbytes, b.owned = ctx, ptr, nbytes, False
        return b

    def upload(self, host: np.ndarray, offset: int = 0):
        host = np.ascontiguousarray(host)
        assert offset + host.nbytes <= self.nbytes
        check(self.ctx.lib.gnsship_dev_upload(self.ctx.h, self.ptr + offset, host.ctypes.data, host.nbytes), "gnsship_dev_upload",
              self.ctx.h)

    def download(self, out: np.ndarray, offset: int = 0):
        assert offset + out.nbytes <= self.nbytes and out.flags.c_contiguous
        check(self.ctx.lib.gnsship_dev_download(self.ctx.h, out.ctypes.data, self.ptr + offset, out.nbytes), "gnsship_dev_download",
              self.ctx.h)
        return out

    def free(self):
        if self.ptr and self.owned:
            self.ctx.lib.gnsship_dev_free(self.ctx.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
                self.free()
        except Exception:
            pass


def comm_unique_id() -> bytes:
    """A fresh RCCL unique id (rank 0 makes it; the launcher's store carries it to the others)."""
    buf = ctypes.create_string_buffer(abi.COMM_ID_BYTES)
    check(abi.load().gnsship_comm_unique_id(buf), "gnsship_comm_unique_id")
    return buf.raw


class Comm:
    """gnsship_comm: one RCCL communicator per context, collectives on the context stream — the
    multi-GPU form of the flowgraph's conditioner → channels fan-out (gnss_flowgraph.cc:1127-1136)."""

    def __init__(self, ctx: Context, n_ranks: int, rank: int, uid: bytes):
        if len(uid) != abi.COMM_ID_BYTES:
            raise ValueError("RCCL unique id must be 128 bytes")
        self.ctx = ctx
        self.rank, self.n_ranks = rank, n_ranks
        h = ctypes.c_void_p()
        idbuf = ctypes.create_string_buffer(uid, abi.COMM_ID_BYTES)
        check(ctx.lib.gnsship_comm_create(ctx.h, n_ranks, rank, idbuf, ctypes.byref(h)), "gnsship_comm_create", ctx.h)
        self.h = h

    @classmethod
    def from_process_group(cls, ctx: Context):
        """Build the communicator over the ranks of the initialised torch.distributed group: rank 0's
        id travels through the group (any backend), then every rank joins."""
        import torch.distributed as dist
        rank, world = dist.get_rank(), dist.get_world_size()
        obj = [comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        return cls(ctx, world, rank, obj[0])

    def broadcast(self, dev_ptr: int, nbytes: int, root: int = 0):
        check(self.ctx.lib.gnsship_comm_broadcast(self.h, dev_ptr, nbytes, root), "gnsship_comm_broadcast", self.ctx.h)

    def allgather(self, dev_send: int, dev_recv: int, bytes_per_rank: int):
        check(self.ctx.lib.gnsship_comm_allgather(self.h, dev_send, dev_recv, bytes_per_rank), "gnsship_comm_allgather", self.ctx.h)

    def max_f64(self, values) -> np.ndarray:
        """Max over ranks of a few doubles (host in, host out; through a device buffer)."""
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        buf = self.ctx.upload(v)
        check(self.ctx.lib.gnsship_comm_allreduce_max_f64(self.h, buf.ptr, v.size), "gnsship_comm_allreduce_max_f64", self.ctx.h)
        self.ctx.sync()
        out = buf.download(np.empty_like(v))
        buf.free()
        return out

    def close(self):
        if self.h:
            self.ctx.lib.gnsship_comm_destroy(self.h)
            self.h = None


class _Handle:
    """What every handle class shares over the C ABI (gnsship_<block>_*): the context, the handle and its life cycle.
    A subclass states its C prefix, sets ``ctx`` and opens the handle with _create in __init__, and makes every other
    call through _call, which raises GnssHipError under the C function's name with the context's last error."""
    _prefix = None  # "gnsship_trk"

    def _call(self, name: str, *args):
        name = f"{self._prefix}_{name}"
        check(getattr(self.ctx.lib, name)(self.h, *args), name, self.ctx.h)

    def _create(self, *args):
        """gnsship_<block>_create(ctx, *args, &handle)"""
        h = ctypes.c_void_p()
        name = f"{self._prefix}_create"
        check(getattr(self.ctx.lib, name)(self.ctx.h, *args, ctypes.byref(h)), name, self.ctx.h)
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.ctx.lib, f"{self._prefix}_destroy")(self.h)
            self.h = None

    def __del__(self):
        try:
            if self.h and self.ctx.h:  # a closed context has taken its handles with it
                self.close()
        except Exception:
            pass


def _if_input(sig, fmt):
    """IF samples as the run calls take them: a host ndarray (CF32 / CI16 / CI8 by its dtype) or a DeviceBuffer (then
    fmt, CF32 when None).  Returns (pointer, on_device, fmt, n_samples); a host pointer keeps its array alive."""
    if isinstance(sig, DeviceBuffer):
        ptr, on_dev, f = sig.ptr, 1, FMT_CF32 if fmt is None else fmt
    else:
        sig = np.ascontiguousarray(sig)
        ptr, on_dev, f = sig.ctypes.data_as(ctypes.c_void_p), 0, sample_format(sig)
    return ptr, on_dev, f, sig.nbytes // _FMT_BYTES[f] if f in _FMT_BYTES else None


class MultiCorrelatorRealCodes(_Handle):
    """Mirror of Cpu_Multicorrelator_Real_Codes (cpu_multicorrelator_real_codes.h:37-61).  rotator: the
    volk_gnsssdr rotator variant its Carrier_wipeoff_multicorrelator_resampler runs (abi.ROTATOR_*;
    default AUTO = what the reference's dispatcher picks on this host)."""

    _prefix = "gnsship_corr"

    def __init__(self, ctx: Context, rotator: int = abi.ROTATOR_AUTO):
        self.ctx = ctx
        self.rotator = rotator
        self.h = None
        self.n_correlators = 0
        self._out = None
        self._sig = None

    def init(self, max_signal_length_samples: int, n_correlators: int) -> bool:
        self._create(max_signal_length_samples, n_correlators)
        self.n_correlators = n_correlators
        self._call("set_rotator", self.rotator)
        return True

    def set_high_dynamics_resampler(self, use: bool):
        self._call("set_high_dynamics_resampler", int(use))

    def set_local_code_and_taps(self, code_length_chips: int, local_code_in: np.ndarray, shifts_chips: np.ndarray) -> bool:
        code = np.ascontiguousarray(local_code_in[:code_length_chips], np.float32)
        shifts = np.ascontiguousarray(shifts_chips, np.float32)
        if len(shifts) < self.n_correlators:
            raise ValueError("need one shift per correlator")
        self._call("set_local_code_and_taps", code_length_chips, fptr(code), fptr(shifts))
        return True

    def set_input_output_vectors(self, corr_out: np.ndarray, sig_in: np.ndarray) -> bool:
        self._out = corr_out
        self._sig = sig_in
        return True

    def Carrier_wipeoff_multicorrelator_resampler(self, rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad,
                                                  rem_code_phase_chips, code_phase_step_chips, code_phase_rate_step_chips,
                                                  signal_length_samples) -> bool:
        sig = np.ascontiguousarray(self._sig)
        fmt = sample_format(sig)
        tmp = np.zeros(2 * self.n_correlators, np.float32)
        self._call("run", sig.ctypes.data, fmt, 0, rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad, rem_code_phase_chips,
                   code_phase_step_chips, code_phase_rate_step_chips, signal_length_samples, fptr(tmp))
        self._out[: self.n_correlators] = tmp.view(np.complex64)
        return True

    def free(self) -> bool:
        self.close()
        return True


class CorrelatorBatch(_Handle):
    """Batched multicorrelator: every row of a JOB_DTYPE array is one channel-epoch."""
    _prefix = "gnsship_batch"

    def __init__(self, ctx: Context, max_jobs: int):
        self.ctx = ctx
        self._create(max_jobs)
        self.n_jobs = 0

    def set_jobs(self, jobs: np.ndarray, n_buffer_samples: int):
        jobs = np.ascontiguousarray(jobs, JOB_DTYPE)
        self._call("set_jobs", jobs.ctypes.data, len(jobs), n_buffer_samples)
        self.n_jobs = len(jobs)

    def launch(self, samples: DeviceBuffer, fmt: int = FMT_CF32):
        self._call("launch", samples.ptr, fmt)

    def launch_ptr(self, dev_ptr: int, fmt: int = FMT_CF32, stages: int = 3):
        self._call("launch_stages", dev_ptr, fmt, stages)

    def launch_pipelined(self, dev_ptr: int, fmt: int = FMT_CF32, next_batch: "CorrelatorBatch" = None,
                         next2: "CorrelatorBatch" = None):
        """Correlate this batch and, in the same launch, replay anchors of the batches after it
        (gnsship_batch_launch_pipelined2): all of `next_batch`'s remaining replay and the first half
        of `next2`'s.  Pairs alternate A, B, A, ...; rings of three A, B, C, A, ... (with next2)
        carry half a replay chain per batch per launch."""
        nh = next_batch.h if next_batch is not None else None
        n2 = next2.h if next2 is not None else None
        self._call("launch_pipelined2", dev_ptr, fmt, nh, n2)

    def results(self) -> np.ndarray:
        out = np.zeros((self.n_jobs, 2 * MAX_TAPS), np.float32)
        self._call("results", fptr(out))
        return out.view(np.complex64)


def correlate_host(ctx: Context, samples: np.ndarray, jobs: np.ndarray, codes: list) -> np.ndarray:
    """Upload samples + codes, run one batch, return complex64[n_jobs, MAX_TAPS]."""
    fmt = sample_format(samples)
    for i, c in enumerate(codes):
        ctx.set_code(i, c)
    buf = ctx.upload(samples)
    n_samples = samples.nbytes // _FMT_BYTES[fmt]
    b = CorrelatorBatch(ctx, max(1, len(jobs)))
    try:
        b.set_jobs(jobs, n_samples)
        b.launch(buf, fmt)
        return b.results()
    finally:
        b.close()
        buf.free()


class AcqLayout(NamedTuple):
    """The transform layout of an acquisition handle (gnsship_acq_layout): N = P × row_len."""
    kind: str       # "lds" (one workgroup, P = 0), "four_step" or "huge"
    P: int          # register points per column; 0 for "lds"
    row_len: int    # M, the LDS transform's length (N for "lds")
    radix: tuple    # Stockham radices of the row plan, in pass order
    ct_rows: bool   # the rows run a kernel with a compile-time plan


class PcpsAcquisition(_Handle):
    """pcps_acquisition (pcps_acquisition.cc) over up to ``max_prns`` local codes at once."""
    _prefix = "gnsship_acq"

    def __init__(self, ctx: Context, fs_in: int, fft_size: int, doppler_max: int, doppler_step: int, doppler_center: int = 0,
                 use_cfar: bool = True, samples_per_chip: int = None, samples_per_code: float = None, max_prns: int = 1,
                 max_dwells: int = 1, chip_rate: float = 1023000.0, ms_per_code: int = 1, consumed_samples: int = 0,
                 bit_transition_flag: bool = False, resampler_ratio: float = 1.0, resampler_latency_samples: int = 0):
        self.ctx = ctx
        conf = abi.AcqConf()
        conf.fs_in = fs_in
        conf.fft_size = fft_size
        conf.doppler_max = doppler_max
        conf.doppler_step = doppler_step
        conf.doppler_center = doppler_center
        conf.max_dwells = max_dwells
        conf.use_cfar = int(use_cfar)
        # Acq_Conf::SetDerivedParams (acq_conf.cc:113-118), float arithmetic as in the reference
        spms = np.float32(np.float32(fs_in) * np.float32(0.001))
        conf.samples_per_chip = int(np.ceil(np.float32(fs_in) / np.float32(chip_rate))) if samples_per_chip is None else samples_per_chip
        conf.samples_per_code = float(np.float32(spms * np.float32(ms_per_code))) if samples_per_code is None else samples_per_code
        conf.max_prns = max_prns
        conf.consumed_samples = consumed_samples
        conf.bit_transition_flag = int(bit_transition_flag)
        conf.resampler_ratio = resampler_ratio
        conf.resampler_latency_samples = resampler_latency_samples
        self.conf = conf
        self.consumed = consumed_samples or fft_size
        self.code_len = fft_size // 2 if bit_transition_flag else self.consumed  # samples set_local_code reads
        self.row_len = fft_size // 2 if bit_transition_flag else fft_size       # grid row length
        self._create(ctypes.byref(conf))
        self._refresh_bins()
        self.fdma_channels = 0  # > 0: the grid is an FDMA grid (set_grid_fdma)

    def _refresh_bins(self):
        nb = ctypes.c_int()
        self._call("num_bins", ctypes.byref(nb))
        self.n_bins = nb.value

    @property
    def layout(self) -> AcqLayout:
        """The transform layout the handle chose at create (gnsship_acq_layout_get)."""
        lay = abi.AcqLayout()
        self._call("layout_get", ctypes.byref(lay))
        return AcqLayout(("lds", "four_step", "huge")[lay.kind], lay.P, lay.row_len, tuple(lay.radix[: lay.n_passes]), bool(lay.ct_rows))

    def set_grid(self, doppler_max: int, doppler_step: int, doppler_center: int = 0):
        self._call("set_grid", doppler_max, doppler_step, doppler_center)
        self._refresh_bins()
        self.fdma_channels = 0

    def set_grid_step2(self, doppler_center_step_two: float, doppler_step2: float, num_doppler_bins_step2: int,
                       step_one_input_power: float):
        """update_grid_doppler_wipeoffs_step2 (pcps_acquisition.cc:305-312): make_2_steps' narrow grid."""
        self._call("set_grid_step2", doppler_center_step_two, doppler_step2, num_doppler_bins_step2, step_one_input_power)
        self._refresh_bins()

    def set_local_code(self, code: np.ndarray, prn_slot: int = 0):
        code = np.ascontiguousarray(code, np.complex64)
        if len(code) < self.code_len:
            raise ValueError(f"local code must have at least {self.code_len} samples")
        code = np.ascontiguousarray(code[: self.code_len])
        self._call("set_local_code", prn_slot, fptr(code.view(np.float32)))

    def run(self, sig, n_prns: int = 1, want_grid: bool = False, fmt: int = None):
        """sig: host ndarray (CF32/CI16/CI8) or DeviceBuffer (then pass fmt)."""
        res = (abi.AcqResult * n_prns)()
        grid = np.zeros((n_prns, self.n_bins, self.row_len), np.float32) if want_grid else None
        ptr, on_dev, f, _ = _if_input(sig, fmt)
        self._call("run", ptr, f, on_dev, n_prns, res, fptr(grid) if want_grid else None)
        return list(res), grid

    def set_grid_fdma(self, doppler_max: int, doppler_step: int, doppler_center: int, bias_hz):
        """One Doppler grid per FDMA frequency channel (pcps_acquisition's d_doppler_bias, :211-229, :295-302):
        channel g's rows are built from bias_hz[g] + the grid's Doppler.  set_grid returns to the ordinary grid."""
        bias = np.ascontiguousarray(bias_hz, np.int32)
        self._call("set_grid_fdma", doppler_max, doppler_step, doppler_center, len(bias), bias.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        self._refresh_bins()
        self.fdma_channels = len(bias)

    def run_fdma(self, sig, prn_slot: int = 0, want_grid: bool = False, fmt: int = None):
        """One dwell of the code in prn_slot under every channel of the FDMA grid: one result per channel (its
        doppler_hz without the bias) and, with want_grid, the grid as (channels, n_bins, row_len)."""
        nch = self.fdma_channels
        if not nch:
            raise ValueError("run_fdma needs set_grid_fdma first")
        res = (abi.AcqResult * nch)()
        grid = np.zeros((nch, self.n_bins, self.row_len), np.float32) if want_grid else None
        ptr, on_dev, f, _ = _if_input(sig, fmt)
        self._call("run_fdma", ptr, f, on_dev, prn_slot, res, fptr(grid) if want_grid else None)
        return list(res), grid


def _ms_code_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, code_rate_cps, code_length_chips, kw) -> PcpsAcquisition:
    """The acquisition of a signal whose code lasts 1 ms: ms_per_code 1, code_length = floor(fs / codes per second)
    samples and a search window of sampled_ms of them."""
    code_length = int(np.floor(fs_in / (code_rate_cps / code_length_chips)))
    return PcpsAcquisition(ctx, fs_in, sampled_ms * code_length, doppler_max, doppler_step, chip_rate=code_rate_cps, ms_per_code=1, **kw)


def _vector_length(fs_in, code_rate_cps, code_length_chips) -> int:
    """A tracking block's vector_length: round(fs / codes per second) samples."""
    return int(round(fs_in / (code_rate_cps / code_length_chips)))


def _glonass_pcps_acquisition(signal, ctx, fs_in, doppler_max, doppler_step, freq_channels, sampled_ms, kw):
    from . import codes
    acq = _ms_code_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, codes.GLONASS_L1_CA_CODE_RATE_CPS,
                               codes.GLONASS_L1_CA_CODE_LENGTH_CHIPS, kw)
    acq.freq_channels = [int(k) for k in freq_channels]
    # gnsship_acq_create has just built the ordinary grid's table and buffers; they are replaced here, once per handle
    # (a few ms of host table per grid).  Kept so: a handle is always runnable, and creation is not on the dwell path.
    acq.set_grid_fdma(doppler_max, doppler_step, kw.get("doppler_center", 0), [codes.glonass_doppler_bias_hz(signal, k) for k in acq.freq_channels])
    acq.set_local_code(codes.glonass_l1_ca_acquisition_code(fs_in, sampled_ms))
    return acq


def glonass_l1_ca_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, freq_channels=range(-7, 7),
                                   sampled_ms: int = 1, **kw) -> PcpsAcquisition:
    """GlonassL1CaPcpsAcquisition's parameters (glonass_l1_ca_pcps_acquisition.cc:49-66): ms_per_code 1, the C/A chip
    rate 511 kcps, code_length = floor(fs / 1000) samples and a search window of sampled_ms of them (an optimum
    acquisition rate of 100e6: no resampler is ever designed).  Every satellite sends the same code, so the handle
    comes back with that code in slot 0 and the FDMA grid of freq_channels set (bias (int32)(DFRQ1_GLO · k), as
    is_fdma() computes it): run_fdma(sig) gives one result per entry of acq.freq_channels.  The channel of a PRN is
    codes.glonass_freq_channel(prn).  Other PcpsAcquisition arguments pass through."""
    return _glonass_pcps_acquisition("1G", ctx, fs_in, doppler_max, doppler_step, freq_channels, sampled_ms, kw)


def glonass_l2_ca_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, freq_channels=range(-7, 7),
                                   sampled_ms: int = 1, **kw) -> PcpsAcquisition:
    """GlonassL2CaPcpsAcquisition (glonass_l2_ca_pcps_acquisition.cc:48-66): as L1 with the bias (int32)(DFRQ2_GLO · k)."""
    return _glonass_pcps_acquisition("2G", ctx, fs_in, doppler_max, doppler_step, freq_channels, sampled_ms, kw)


def _glonass_trk_conf(system: int, fs_in: float, kw) -> "abi.TrkConf":
    from . import codes
    vl = _vector_length(fs_in, codes.GLONASS_L1_CA_CODE_RATE_CPS, codes.GLONASS_L1_CA_CODE_LENGTH_CHIPS)
    base = dict(pll_bw_hz=50.0, dll_bw_hz=2.0, early_late_space_chips=0.5, max_carrier_lock_fail=50, rotator=abi.ROTATOR_GENERIC)
    base.update(kw)
    return abi.TrkConf.defaults(system, fs_in, vl, **base)


def glonass_l1_ca_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GlonassL1CaDllPllTracking's configuration (glonass_l1_ca_dll_pll_tracking.cc:44-62): vector_length = round(fs / 1000),
    pll_bw_hz 50, dll_bw_hz 2, early_late_space_chips 0.5; max_carrier_lock_fail carries the block's gflag max_lock_fail (50),
    carrier_lock_th and cn0_min theirs (0.7, 25).  The rotator is the generic one (the only one the engine has for this
    block).  Tracking code: codes.glonass_l1_ca_code_gen_float(); start's prn selects the frequency channel."""
    return _glonass_trk_conf(abi.SYS_GLO_L1CA, fs_in, kw)


def glonass_l2_ca_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GlonassL2CaDllPllTracking (glonass_l2_ca_dll_pll_tracking.cc:44-62): as L1 on the L2 carrier and spacing."""
    return _glonass_trk_conf(abi.SYS_GLO_L2CA, fs_in, kw)


def gps_l5i_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, sampled_ms: int = 1, **kw) -> PcpsAcquisition:
    """GpsL5iPcpsAcquisition's parameters (gps_l5i_pcps_acquisition.cc:49-69): ms_per_code 1, the L5I
    chip rate, code_length = floor(fs / 1000) samples and a search window of sampled_ms of them.
    The local code is codes.gps_l5i_acquisition_code(prn, fs_in, sampled_ms); a front end faster than
    codes.GPS_L5_OPT_ACQ_FS_SPS designs its resampler with acq_resampler_design(lib, fs, that rate)
    and passes the resampled rate here.  Other PcpsAcquisition arguments pass through."""
    from . import codes
    return _ms_code_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, codes.GPS_L5I_CODE_RATE_CPS, codes.GPS_L5I_CODE_LENGTH_CHIPS, kw)


def gps_l5_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GpsL5DllPllTracking's configuration (gps_l5_dll_pll_tracking.cc:44-65): vector_length =
    round(fs / 1000), the L5Q pilot tracked (track_pilot = 1; data-only tracking is rejected by
    gnsship_trk_create), extend_correlation_symbols at least 1.  Tracking code: codes.gps_l5q_code_gen_float,
    data code (start's data_code_id): codes.gps_l5i_code_gen_float."""
    from . import codes
    vl = _vector_length(fs_in, codes.GPS_L5I_CODE_RATE_CPS, codes.GPS_L5I_CODE_LENGTH_CHIPS)
    c = abi.TrkConf.defaults(abi.SYS_GPS_L5, fs_in, vl, **kw)
    if c.extend_correlation_symbols < 1:
        c.extend_correlation_symbols = 1
    return c


def beidou_b3i_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, sampled_ms: int = 1, **kw) -> PcpsAcquisition:
    """BeidouB3iPcpsAcquisition's parameters (beidou_b3i_pcps_acquisition.cc:46-63): ms_per_code 1, the B3I
    chip rate, code_length = floor(fs / 1000) samples and a search window of sampled_ms of them.  The
    reference passes an optimum acquisition rate of 100e6, so no resampler is ever designed.  The local
    code is codes.beidou_b3i_acquisition_code(prn, fs_in, sampled_ms)."""
    from . import codes
    return _ms_code_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, codes.BEIDOU_B3I_CODE_RATE_CPS,
                                codes.BEIDOU_B3I_CODE_LENGTH_CHIPS, kw)


def gps_l2_m_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, sampled_ms: int = 20, **kw) -> PcpsAcquisition:
    """GpsL2MPcpsAcquisition's parameters (gps_l2_m_pcps_acquisition.cc:50-78): ms_per_code 20, the L2 CM
    chip rate, code_length = floor(fs / 50) samples, a search window of floor(sampled_ms · samples_per_ms)
    samples holding sampled_ms / 20 codes (samples_per_code = samples_per_ms · 20).  The local code is
    codes.gps_l2c_m_acquisition_code(prn, fs_in, sampled_ms); a front end faster than
    codes.GPS_L2C_OPT_ACQ_FS_SPS designs its resampler with acq_resampler_design(lib, fs, that rate) and
    passes the resampled rate here."""
    from . import codes
    spms = np.float32(np.float32(fs_in) * np.float32(0.001))
    return PcpsAcquisition(ctx, fs_in, int(np.floor(np.float32(sampled_ms) * spms)), doppler_max, doppler_step,
                           chip_rate=codes.GPS_L2_M_CODE_RATE_CPS, ms_per_code=20, **kw)


def beidou_b3i_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """BeidouB3iDllPllTracking's configuration (beidou_b3i_dll_pll_tracking.cc): vector_length =
    round(fs / 1000), extend_correlation_symbols within [1, 20] (a GEO channel — start's prn in 1..5 or
    above 58 — is further capped at 2 by the engine).  Tracking code: codes.beidou_b3i_code_gen_float."""
    from . import codes
    vl = _vector_length(fs_in, codes.BEIDOU_B3I_CODE_RATE_CPS, codes.BEIDOU_B3I_CODE_LENGTH_CHIPS)
    c = abi.TrkConf.defaults(abi.SYS_BDS_B3I, fs_in, vl, **kw)
    c.extend_correlation_symbols = min(max(c.extend_correlation_symbols, 1), 20)
    c.track_pilot = 0
    return c


def gps_l2c_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GpsL2MDllPllTracking's configuration (gps_l2_m_dll_pll_tracking.cc:44-62): vector_length =
    round(fs / 50) — one 20 ms L2 CM code period, which is one telemetry symbol —
    extend_correlation_symbols = 1 and track_pilot = 0 (the signal has no pilot).  The reference's L2C
    configurations run the loops at pll_bw_hz = 2, dll_bw_hz = 0.25: Dll_Pll_Conf's defaults (35 / 2 Hz)
    are unstable at a 20 ms update interval.  Tracking code: codes.gps_l2c_m_code_gen_float."""
    from . import codes
    vl = _vector_length(fs_in, codes.GPS_L2_M_CODE_RATE_CPS, codes.GPS_L2_M_CODE_LENGTH_CHIPS)
    c = abi.TrkConf.defaults(abi.SYS_GPS_L2C, fs_in, vl, **kw)
    c.extend_correlation_symbols = 1
    c.track_pilot = 0
    return c


def _e5_pcps_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, kw):
    from . import codes
    return _ms_code_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, codes.GALILEO_E5A_CODE_CHIP_RATE_CPS,
                                codes.GALILEO_E5A_CODE_LENGTH_CHIPS, kw)


def galileo_e5a_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, sampled_ms: int = 1,
                                 acquire_pilot: bool = False, acquire_iq: bool = False, **kw) -> PcpsAcquisition:
    """GalileoE5aPcpsAcquisition's parameters (galileo_e5a_pcps_acquisition.cc:48-76): ms_per_code 1, the E5a chip
    rate, code_length = floor(fs / 1000) samples and a search window of sampled_ms of them.  The local code is
    codes.galileo_e5a_acquisition_code(prn, fs_in, sampled_ms, acquire_pilot, acquire_iq) — the sampled "5I" code,
    "5Q" with acquire_pilot, "5X" with acquire_iq (which overrides acquire_pilot, :152-180); the two flags are
    kept on the returned object so that callers build the matching code.  A front end faster than
    codes.GALILEO_E5A_OPT_ACQ_FS_SPS designs its resampler with acq_resampler_design(lib, fs, that rate) and
    passes the resampled rate here, as for GPS L5."""
    acq = _e5_pcps_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, kw)
    acq.acquire_iq = bool(acquire_iq)
    acq.acquire_pilot = bool(acquire_pilot) and not acq.acquire_iq
    return acq


def galileo_e5b_pcps_acquisition(ctx: Context, fs_in: int, doppler_max: int, doppler_step: int, sampled_ms: int = 1,
                                 acquire_pilot: bool = False, acquire_iq: bool = False, **kw) -> PcpsAcquisition:
    """GalileoE5bPcpsAcquisition's parameters: galileo_e5a_pcps_acquisition's twin with the "7I" / "7Q" / "7X" codes
    (codes.galileo_e5b_acquisition_code) and codes.GALILEO_E5B_OPT_ACQ_FS_SPS."""
    acq = _e5_pcps_acquisition(ctx, fs_in, doppler_max, doppler_step, sampled_ms, kw)
    acq.acquire_iq = bool(acquire_iq)
    acq.acquire_pilot = bool(acquire_pilot) and not acq.acquire_iq
    return acq


def _e5_trk_conf(system: int, i_secondary_len: int, fs_in: float, kw) -> "abi.TrkConf":
    from . import codes
    vl = _vector_length(fs_in, codes.GALILEO_E5A_CODE_CHIP_RATE_CPS, codes.GALILEO_E5A_CODE_LENGTH_CHIPS)
    kw.setdefault("track_pilot", 1)
    c = abi.TrkConf.defaults(system, fs_in, vl, **kw)
    c.extend_correlation_symbols = max(c.extend_correlation_symbols, 1)
    if not c.track_pilot:
        c.extend_correlation_symbols = min(c.extend_correlation_symbols, i_secondary_len)
    return c


def galileo_e5a_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GalileoE5aDllPllTracking's configuration (galileo_e5a_dll_pll_tracking.cc:47-58): vector_length =
    round(fs / 1000), extend_correlation_symbols at least 1 and, in data-only mode (track_pilot = 0), at most
    the 20 chips of the I secondary code.  track_pilot = 1 (the default here): tracking code
    codes.galileo_e5a_q_code_gen_float, data code (start's data_code_id) codes.galileo_e5a_i_code_gen_float, and
    start's prn selects the pilot's secondary code.  track_pilot = 0: tracking code the I primary."""
    return _e5_trk_conf(abi.SYS_GAL_E5A, 20, fs_in, kw)


def galileo_e5b_trk_conf(fs_in: float, **kw) -> "abi.TrkConf":
    """GalileoE5bDllPllTracking's configuration: as galileo_e5a_trk_conf with the E5b codes and the 4-chip I
    secondary code (4 symbols per bit)."""
    return _e5_trk_conf(abi.SYS_GAL_E5B, 4, fs_in, kw)


def _design_taps(fn, name: str, *args, refused: str = None) -> np.ndarray:
    """The taps of a design function fn(*args, taps, taps_cap, &n_taps): one call without room for the size (an error
    there reads `refused`, where given), then, when there are taps, one that fills them.  Only gnsship_acq_resampler_design
    succeeds with no taps (no resampler needed); the low-pass designs have at least one."""
    n = ctypes.c_int()
    check(fn(*args, None, 0, ctypes.byref(n)), refused or name)
    taps = np.zeros(n.value, np.float32)
    if n.value:
        check(fn(*args, fptr(taps), len(taps), ctypes.byref(n)), name)
    return taps


def firdes_low_pass(lib, gain: float, fs: float, cutoff: float, transition: float) -> np.ndarray:
    """gr::filter::firdes::low_pass (Hamming) as the library restates it."""
    return _design_taps(lib.gnsship_firdes_low_pass, "gnsship_firdes_low_pass", gain, fs, cutoff, transition,
                        refused="gnsship_firdes_low_pass: bad arguments")


def acq_resampler_design(lib, fs_in: int, opt_acq_fs: float):
    """gnss_flowgraph.cc:1070-1113: (decimation, taps); decimation 1 and no taps when not needed."""
    d = ctypes.c_int()
    taps = _design_taps(lib.gnsship_acq_resampler_design, "gnsship_acq_resampler_design", fs_in, opt_acq_fs, ctypes.byref(d))
    return d.value, taps


class AcqResampler(_Handle):
    """The acquisition resampler FIR (fir_filter_ccf(decimation, taps)) over a sample stream."""
    _prefix = "gnsship_acq_resampler"

    def __init__(self, ctx: Context, taps: np.ndarray, decimation: int, max_in_samples: int):
        self.ctx = ctx
        self.taps = np.ascontiguousarray(taps, np.float32)
        self.decimation = decimation
        self._create(fptr(self.taps), len(self.taps), decimation, max_in_samples)

    @property
    def latency(self) -> int:
        return (len(self.taps) - 1) // 2

    def run(self, x, fmt: int = None, on_device: bool = False, n_in: int = None):
        """Filter a host array (or a device pointer with on_device=True and n_in): returns the
        decimated complex64 samples (host arrays) or (device pointer, n_out)."""
        dev = ctypes.c_void_p()
        n_out = ctypes.c_int64()
        if on_device:
            self._call("run", x, fmt, 1, n_in, None, ctypes.byref(dev), ctypes.byref(n_out))
            return dev.value, n_out.value
        fmt = sample_format(x) if fmt is None else fmt
        n = len(x) if x.dtype == np.complex64 else len(x) // 2
        out = np.zeros(n // self.decimation, np.complex64)
        self._call("run", x.ctypes.data, fmt, 0, n, fptr(out.view(np.float32)), ctypes.byref(dev), ctypes.byref(n_out))
        return out

    def reset(self):
        self._call("reset")


def cond_lowpass_taps(lib, fs: float, decimation: int, bw: float = 0.0, tw: float = 0.0) -> np.ndarray:
    """The Freq_Xlating_Fir_Filter adapter's filter_type=lowpass taps (freq_xlating_fir_filter.cc:99-106):
    firdes::low_pass(1, fs, bw, tw), bw = 0 → (fs / decimation) / 2, tw = 0 → bw / 10."""
    return _design_taps(lib.gnsship_cond_lowpass_taps, "gnsship_cond_lowpass_taps", fs, decimation, bw, tw,
                        refused="gnsship_cond_lowpass_taps: bad arguments")


class SignalConditioner(_Handle):
    """The signal conditioner's frequency-translating FIR decimator (freq_xlating_fir_filter_ccf(decimation,
    taps, IF, fs) per band) over one sample stream.  bands: [(if_hz, decimation, taps), ...], up to 4."""
    _prefix = "gnsship_cond"

    def __init__(self, ctx: Context, fs_in: float, bands, max_in_samples: int):
        self.ctx = ctx
        self.fs_in = fs_in
        self.bands = [(float(f), int(d), np.ascontiguousarray(t, np.float32)) for f, d, t in bands]
        arr = (abi.CondBand * max(1, len(self.bands)))()
        for i, (f, d, t) in enumerate(self.bands):
            arr[i] = abi.CondBand(if_hz=f, decimation=d, taps=fptr(t), n_taps=len(t))
        self._create(fs_in, arr, len(self.bands), max_in_samples)

    @property
    def n_bands(self) -> int:
        return len(self.bands)

    def run(self, x, fmt: int = None, on_device: bool = False, n_in: int = None, dev_dst=None, host: bool = None):
        """Filter a host array, or a device pointer with on_device=True, fmt and n_in.  fmt defaults to the
        array's complex format (sample_format); a real float32 / int16 / int8 array needs fmt=FMT_RF32 /
        FMT_RI16 / FMT_RI8 and a uint8 array of packed bytes a packed fmt (abi.fmt_packed and the presets),
        n_in then defaulting to bytes × samples per byte.  dev_dst: per-band device pointers (None entries
        = the handle's own buffers).  Returns the list of per-band complex64 arrays when host (the default
        for a host input), else [(device pointer, n_out), ...]."""
        nb = self.n_bands
        if on_device:
            ptr = ctypes.c_void_p(x)
        else:
            x = np.ascontiguousarray(x)
            fmt = sample_format(x) if fmt is None else fmt
            if n_in is None:
                bits = self.ctx.lib.gnsship_cond_fmt_bits(fmt)
                if bits <= 0:
                    raise ValueError(f"SignalConditioner.run: unknown sample format {fmt}")
                n_in = x.nbytes * 8 // bits
            ptr = ctypes.c_void_p(x.ctypes.data)
        host = (not on_device) if host is None else host
        dst = None
        if dev_dst is not None:
            dst = (ctypes.c_void_p * nb)(*[int(p) if p else None for p in dev_dst])
        dev = (ctypes.c_void_p * nb)()
        n_out = (ctypes.c_int64 * nb)()
        outs, hp = None, None
        if host:
            outs = [np.zeros(max(0, n_in // d), np.complex64) for _, d, _ in self.bands]
            hp = (abi._f32p * nb)(*[fptr(o.view(np.float32)) for o in outs])
        self._call("run", ptr, fmt, int(on_device), n_in, dst, hp, dev, n_out)
        self.last_dev = [(dev[b], n_out[b]) for b in range(nb)]
        return outs if host else self.last_dev

    def reset(self, first_sample: int = 0):
        self._call("reset", first_sample)

    def samples_in(self) -> int:
        n = ctypes.c_uint64()
        self._call("samples_in", ctypes.byref(n))
        return n.value


def mit_threshold(lib, pfa: float, length: int) -> float:
    """thres_ of the three mitigation blocks: the upper pfa quantile of chi²(2·length), as a float32 value."""
    t = ctypes.c_float()
    rc = lib.gnsship_mit_threshold(pfa, length, ctypes.byref(t))
    if rc != abi.OK:
        raise abi.GnssHipError(rc, "gnsship_mit_threshold: pfa in (0, 1), length in 2..1024")
    return t.value


class InterferenceMitigation(_Handle):
    """Pulse blanking, notch or notch-lite filter (pulse_blanking_cc / notch_cc / notch_lite_cc) over one CF32
    stream.  kind: "pulse-blanking" | "notch" | "notch-lite" or abi.MIT_*; chain_form: "auto" | "serial" |
    "speculative" or abi.MIT_CHAIN_*.  A run returns the complete segments not yet emitted; the rest stays on
    the device."""

    _prefix = "gnsship_mit"
    KINDS = {"pulse-blanking": abi.MIT_PULSE_BLANKING, "notch": abi.MIT_NOTCH, "notch-lite": abi.MIT_NOTCH_LITE}
    FORMS = {"auto": abi.MIT_CHAIN_AUTO, "serial": abi.MIT_CHAIN_SERIAL, "speculative": abi.MIT_CHAIN_SPECULATIVE}

    def __init__(self, ctx: Context, kind, max_in_samples: int, pfa: float = None, threshold: float = 0.0, p_c_factor: float = 0.9,
                 length: int = 32, n_segments_est: int = 12500, n_segments_reset: int = 5000000, n_segments_coeff: int = 1,
                 chain_form="auto"):
        self.ctx = ctx
        self.h = None
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        if pfa is None:  # the adapters' defaults
            pfa = 0.04 if self.kind == abi.MIT_PULSE_BLANKING else 0.001
        form = self.FORMS[chain_form] if isinstance(chain_form, str) else int(chain_form)
        self.conf = abi.MitConf(kind=self.kind, pfa=pfa, threshold=threshold, p_c_factor=p_c_factor, length=length,
                                n_segments_est=n_segments_est, n_segments_reset=n_segments_reset, n_segments_coeff=n_segments_coeff,
                                chain_form=form)
        self.max_in_samples = int(max_in_samples)
        self._create(ctypes.byref(self.conf), self.max_in_samples)
        self._pending = 0

    def run(self, x, on_device: bool = False, n_in: int = None, dev_dst=None, host: bool = None):
        """Filter a host complex64 array, or a device pointer with on_device=True and n_in.  Returns the
        emitted samples as a complex64 array when host (the default for a host input), else (device
        pointer, n_out)."""
        if on_device:
            ptr = ctypes.c_void_p(x)
        else:
            x = np.ascontiguousarray(x, np.complex64)
            n_in = x.size if n_in is None else n_in
            ptr = ctypes.c_void_p(x.ctypes.data) if x.size else None
        host = (not on_device) if host is None else host
        out = np.zeros(max(0, self._pending + n_in), np.complex64) if host else None
        dev = ctypes.c_void_p()
        n_out = ctypes.c_int64()
        self._call("run", ptr, int(on_device), n_in, ctypes.c_void_p(dev_dst) if dev_dst else None,
                   fptr(out.view(np.float32)) if host and out.size else None, ctypes.byref(dev), ctypes.byref(n_out))
        self._pending += n_in - n_out.value
        self.last_dev = (dev.value, n_out.value)
        return out[:n_out.value] if host else self.last_dev

    def reset(self):
        self._call("reset")
        self._pending = 0

    def state(self) -> dict:
        st = abi.MitState()
        self._call("state_get", ctypes.byref(st))
        return {name: getattr(st, name) for name, _ in abi.MitState._fields_}


class ViterbiDecoder(_Handle):
    """The K = 7, rate-1/2 Viterbi decoder of the Galileo telemetry block with its de-interleaver and G2 flip
    (galileo_telemetry_decoder_gs.cc:342-371, viterbi_decoder.cc:47-120) for up to ``max_channels`` channels, one
    Viterbi_Decoder object per channel.  mode: "reference" (the decoder as written: first symbol of each pair only,
    metrics carried from frame to frame) | "full" (both symbols, every frame from state 0) or abi.VIT_MODE_*."""

    _prefix = "gnsship_vit"
    MODES = {"reference": abi.VIT_MODE_REFERENCE, "full": abi.VIT_MODE_FULL}

    def __init__(self, ctx: Context, max_channels: int, data_length: int, interleaver_rows: int = 0, interleaver_cols: int = 0,
                 invert_g2: bool = False, mode="reference", g=(121, 91), constraint_length: int = 7, rate_n: int = 2):
        self.ctx = ctx
        self.h = None
        self.mode = self.MODES[mode] if isinstance(mode, str) else int(mode)
        self.conf = abi.VitConf(constraint_length=constraint_length, rate_n=rate_n, g=(ctypes.c_int32 * 2)(int(g[0]), int(g[1])),
                                data_length=data_length, interleaver_rows=interleaver_rows, interleaver_cols=interleaver_cols,
                                invert_g2=int(bool(invert_g2)), mode=self.mode)
        self.max_channels = int(max_channels)
        self.data_length = int(data_length)
        self.frame_symbols = 2 * (self.data_length + 6)
        self._create(ctypes.byref(self.conf), self.max_channels)

    def run(self, symbols, channels, negate=None, on_device: bool = False, n_frames: int = None, bits_dev=None, host: bool = True):
        """Decode frames: a host float32 array [n_frames, frame_symbols] as received, or a device pointer with
        on_device=True; channels int32[n_frames]; negate uint8[n_frames] or None.  Returns uint8[n_frames,
        data_length] (0 / 1) when host, else None (the bits are at bits_dev, asynchronously)."""
        channels = np.ascontiguousarray(channels, np.int32).ravel()
        n_frames = channels.size if n_frames is None else int(n_frames)
        if channels.size != n_frames:
            raise ValueError("one channel per frame")
        if on_device:
            ptr = ctypes.c_void_p(symbols)
        else:
            symbols = np.ascontiguousarray(symbols, np.float32)
            if symbols.size != n_frames * self.frame_symbols:
                raise ValueError(f"{n_frames} frames of {self.frame_symbols} symbols expected, got {symbols.size} symbols")
            ptr = ctypes.c_void_p(symbols.ctypes.data) if symbols.size else None
        u8p = ctypes.POINTER(ctypes.c_uint8)
        if negate is not None:
            negate = np.ascontiguousarray(negate, np.uint8).ravel()
            if negate.size != n_frames:
                raise ValueError("one negate flag per frame")
        out = np.zeros((n_frames, self.data_length), np.uint8) if host else None
        self._in_flight = (symbols, channels, negate)  # a run without a host copy returns before the stream has read them
        self._call("run", ptr, int(on_device), n_frames, channels.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                   negate.ctypes.data_as(u8p) if negate is not None else None, out.ctypes.data_as(u8p) if host and out.size else None,
                   ctypes.c_void_p(bits_dev) if bits_dev else None)
        return out

    def state(self, channel: int) -> np.ndarray:
        """The channel's 64 carried path metrics (d_prev_section)."""
        sec = np.zeros(64, np.float32)
        self._call("state_get", channel, fptr(sec))
        return sec

    def reset_channel(self, channel: int):
        """A new Viterbi_Decoder object on this channel."""
        self._call("reset_channel", channel)


# (interleaver rows, interleaver columns, data length) of the Galileo page types: 8 rows each, frames of 240, 488
# and 984 symbols (an I/NAV page part, an F/NAV page, a C/NAV page without their preambles), 6 tail bits per frame
GALILEO_INAV_PAGE, GALILEO_FNAV_PAGE, GALILEO_CNAV_PAGE = (8, 30, 114), (8, 61, 238), (8, 123, 486)


def _galileo_page_decoder(ctx, max_channels, page, mode):
    rows, cols, data_length = page
    return ViterbiDecoder(ctx, max_channels, data_length, rows, cols, invert_g2=True, mode=mode)


def galileo_inav_page_decoder(ctx: Context, max_channels: int, mode="reference") -> ViterbiDecoder:
    """decode_INAV_word's first two steps (galileo_telemetry_decoder_gs.cc:354-371): one 240-symbol page part → 114 bits."""
    return _galileo_page_decoder(ctx, max_channels, GALILEO_INAV_PAGE, mode)


def galileo_fnav_page_decoder(ctx: Context, max_channels: int, mode="reference") -> ViterbiDecoder:
    """decode_FNAV_word's first two steps (:585-599): one 488-symbol page → 238 bits."""
    return _galileo_page_decoder(ctx, max_channels, GALILEO_FNAV_PAGE, mode)


def galileo_cnav_page_decoder(ctx: Context, max_channels: int, mode="reference") -> ViterbiDecoder:
    """decode_CNAV_word's first two steps (:684-697): one 984-symbol page → 486 bits."""
    return _galileo_page_decoder(ctx, max_channels, GALILEO_CNAV_PAGE, mode)


class _TelemetryDecoder(_Handle):
    """What the five telemetry decoders share over the C ABI (gnsship_<family>_*, csrc/tlm_host.h): the handle's life
    cycle (_Handle), the three run calls and the device pointers.  A subclass states its C prefix, its result tuple and the name of
    its per-run slot count, builds its configuration in __init__ and its host arrays in _new_result, and adds the calls
    only its family has."""
    _result = None   # the run's NamedTuple; with tow_ms / sflags the family has a per-entry output stream
    _per_run = None  # "subframes_per_run": the attribute holding the record slots per channel of one run
    _state = None    # the ctypes state structure state() reads; a family whose state is a numpy record overrides state()

    def _open(self, ctx: Context, conf, max_channels: int, max_rounds: int):
        self.ctx, self.conf = ctx, conf
        self.max_channels, self.max_rounds = int(max_channels), int(max_rounds)
        self._create(ctypes.byref(conf), self.max_channels)
        slots = ctypes.c_int32()
        self._call("outputs_device", *[None] * len(self._result._fields), ctypes.byref(slots))
        setattr(self, self._per_run, slots.value)

    def _outputs(self, host: bool, n_rounds: int):
        if not host:
            return None, (None,) * len(self._result._fields)
        res = self._new_result(n_rounds)
        return res, tuple(ctypes.c_void_p(x.ctypes.data) for x in res)

    def _run_symbols(self, symbols, masks, on_device, n_rounds, host):
        """masks: ((name, array or device pointer or None), ...) in the C call's order."""
        names, masks = [n for n, _ in masks], [m for _, m in masks]
        if on_device:
            sp = ctypes.c_void_p(symbols)
            ptrs_in = [ctypes.c_void_p(m) if m else None for m in masks]
        else:
            symbols = np.ascontiguousarray(symbols, np.float32).reshape(-1, self.max_channels)
            n_rounds = symbols.shape[0] if n_rounds is None else int(n_rounds)
            sp = ctypes.c_void_p(symbols.ctypes.data) if symbols.size else None
            for i, m in enumerate(masks):
                if m is not None:
                    masks[i] = m = np.ascontiguousarray(m, np.uint8).reshape(-1, self.max_channels)
                    if m.shape != symbols.shape:
                        raise ValueError(f"{names[i]} must have the symbols' shape")
            ptrs_in = [ctypes.c_void_p(m.ctypes.data) if m is not None and m.size else None for m in masks]
        res, ptrs = self._outputs(host, max(0, min(int(n_rounds), self.max_rounds)))
        self._in_flight = (symbols, *masks)  # a run without a host copy returns before the stream has read them
        self._call("run_symbols", sp, *ptrs_in, int(on_device), int(n_rounds), *ptrs)
        return res

    def run_records(self, records, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """records: abi.TRK_EPOCH_DTYPE[n_rounds, max_channels] on the host, or a device pointer with on_device and n_rounds."""
        if on_device:
            rp = ctypes.c_void_p(records)
        else:
            records = np.ascontiguousarray(records, abi.TRK_EPOCH_DTYPE).reshape(-1, self.max_channels)
            n_rounds = records.shape[0] if n_rounds is None else int(n_rounds)
            rp = ctypes.c_void_p(records.ctypes.data) if records.size else None
        res, ptrs = self._outputs(host, max(0, min(int(n_rounds), self.max_rounds)))
        self._in_flight = (records,)
        self._call("run_records", rp, int(on_device), int(n_rounds), *ptrs)
        return res

    def run_trk(self, trk: "DllPllVemlTracking", host: bool = True):
        """Consume, in place, the records the tracker's last run left on the device."""
        res, ptrs = self._outputs(host, self.max_rounds)
        if "tow_ms" not in self._result._fields:
            self._call("run_trk", trk.h, *ptrs)
            return res
        rounds = ctypes.c_int32()
        self._call("run_trk", trk.h, *ptrs, ctypes.byref(rounds))
        if res is None:
            return None
        n = rounds.value  # the copies are dense over the run's rounds
        flat = self.max_rounds * self.max_channels
        return res._replace(tow_ms=res.tow_ms.reshape(flat)[:n * self.max_channels].reshape(n, self.max_channels),
                            sflags=res.sflags.reshape(flat)[:n * self.max_channels].reshape(n, self.max_channels))

    def outputs_device(self):
        """Device pointers of the handle's output buffers, one per field of the result tuple and in its order."""
        p = [ctypes.c_void_p() for _ in self._result._fields]
        self._call("outputs_device", *[ctypes.byref(x) for x in p], None)
        return tuple(x.value for x in p)

    def state(self, channel: int) -> dict:
        """The channel's block members (gnsship_<family>_state) by name."""
        st = self._state()
        self._call("state_get", channel, ctypes.byref(st))
        return st.as_dict()


class TlmResult(NamedTuple):
    """One gnsship_tlm run: pages [max_channels, pages_per_run] (abi.TLM_PAGE_DTYPE), bits uint8[max_channels,
    pages_per_run, LL], counts int32[max_channels], faults uint8[max_channels]; slots k >= counts[c] are unspecified."""
    pages: np.ndarray
    bits: np.ndarray
    counts: np.ndarray
    faults: np.ndarray


class GalileoTelemetryDecoder(_TelemetryDecoder):
    """The frame handling of galileo_telemetry_decoder_gs::general_work (:872-1094) for up to ``max_channels`` channels
    on the device, one block object per channel: preamble synchronisation, page parts, Viterbi, CRC-24Q, the CRC-error
    counter and check_tlm_separation (include/gnsship.h, gnsship_tlm_*).  frame_type abi.TLM_INAV / _FNAV / _CNAV;
    mode "reference" | "full" as ViterbiDecoder; max_rounds: the most symbols per channel one run may carry."""
    _prefix, _result, _per_run, _state = "gnsship_tlm", TlmResult, "pages_per_run", abi.TlmState

    def __init__(self, ctx: Context, frame_type: int, max_channels: int, max_rounds: int, mode="reference"):
        self.frame_type = int(frame_type)
        self.mode = ViterbiDecoder.MODES[mode] if isinstance(mode, str) else int(mode)
        self._open(ctx, abi.TlmConf(frame_type=self.frame_type, vit_mode=self.mode, max_rounds=int(max_rounds), reserved=0), max_channels, max_rounds)
        self.preamble_symbols, self.period, self.required, self.data_length = abi.TLM_GEOMETRY[self.frame_type]

    def _new_result(self, n_rounds: int):
        return TlmResult(np.zeros((self.max_channels, self.pages_per_run), abi.TLM_PAGE_DTYPE),
                         np.zeros((self.max_channels, self.pages_per_run, self.data_length), np.uint8),
                         np.zeros(self.max_channels, np.int32), np.zeros(self.max_channels, np.uint8))

    def run_symbols(self, symbols, valid=None, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """symbols float32[n_rounds, max_channels] (or a device pointer with on_device and n_rounds), valid uint8 of the
        same shape (and place) or None.  Returns a TlmResult, or None when not host (asynchronous)."""
        return self._run_symbols(symbols, (("valid", valid),), on_device, n_rounds, host)

    def reset_channel(self, channel: int):
        """The block's reset()."""
        self._call("reset_channel", channel)

    def set_satellite(self, channel: int):
        """The block's set_satellite()."""
        self._call("set_satellite", channel)

    def new_channel(self, channel: int):
        """A new block object on this channel."""
        self._call("new_channel", channel)


def galileo_inav_telemetry(ctx: Context, max_channels: int, max_rounds: int, mode="reference") -> GalileoTelemetryDecoder:
    """I/NAV (E1-B, E5b-I): 250-symbol page parts, even + odd joined for the CRC."""
    return GalileoTelemetryDecoder(ctx, abi.TLM_INAV, max_channels, max_rounds, mode)


def galileo_fnav_telemetry(ctx: Context, max_channels: int, max_rounds: int, mode="reference") -> GalileoTelemetryDecoder:
    """F/NAV (E5a-I): 500-symbol pages."""
    return GalileoTelemetryDecoder(ctx, abi.TLM_FNAV, max_channels, max_rounds, mode)


def galileo_cnav_telemetry(ctx: Context, max_channels: int, max_rounds: int, mode="reference") -> GalileoTelemetryDecoder:
    """C/NAV frame geometry (E6-B): 1000-symbol pages."""
    return GalileoTelemetryDecoder(ctx, abi.TLM_CNAV, max_channels, max_rounds, mode)


class LnavResult(NamedTuple):
    """One gnsship_lnav run: subframes [max_channels, subframes_per_run] (abi.LNAV_SUBFRAME_DTYPE; slots k >= counts[c] are
    unspecified), counts int32[max_channels], faults uint8[max_channels], and the block's output stream per entry: tow_ms
    uint32[n_rounds, max_channels], sflags uint8[n_rounds, max_channels] (abi.LNAV_S_*), both 0 where the entry is no symbol."""
    subframes: np.ndarray
    counts: np.ndarray
    faults: np.ndarray
    tow_ms: np.ndarray
    sflags: np.ndarray


class GpsL1CaTelemetryDecoder(_TelemetryDecoder):
    """gps_l1_ca_telemetry_decoder_gs up to the time of week for up to ``max_channels`` channels on the device, one block
    object per channel: preamble seeding, subframe synchronisation, the LNAV parity, subframe ID and TOW, the error
    counter, loss of sync, check_tlm_separation and the TOW stamp of every symbol (include/gnsship.h, gnsship_lnav_*).
    max_rounds: the most entries per channel one run may carry."""
    _prefix, _result, _per_run, _state = "gnsship_lnav", LnavResult, "subframes_per_run", abi.LnavState

    def __init__(self, ctx: Context, max_channels: int, max_rounds: int):
        self._open(ctx, abi.LnavConf(max_rounds=int(max_rounds), reserved=0), max_channels, max_rounds)

    def _new_result(self, n_rounds: int):
        return LnavResult(np.zeros((self.max_channels, self.subframes_per_run), abi.LNAV_SUBFRAME_DTYPE),
                          np.zeros(self.max_channels, np.int32), np.zeros(self.max_channels, np.uint8),
                          np.zeros((n_rounds, self.max_channels), np.uint32), np.zeros((n_rounds, self.max_channels), np.uint8))

    def run_symbols(self, symbols, valid=None, flags180=None, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """symbols float32[n_rounds, max_channels] (or a device pointer with on_device and n_rounds); valid and flags180
        uint8 of the same shape (and place) or None.  Returns an LnavResult, or None when not host (asynchronous)."""
        return self._run_symbols(symbols, (("valid", valid), ("flags180", flags180)), on_device, n_rounds, host)

    def reset_channel(self, channel: int):
        """The block's reset()."""
        self._call("reset_channel", channel)

    def set_satellite(self, channel: int):
        """The block's set_satellite()."""
        self._call("set_satellite", channel)

    def new_channel(self, channel: int):
        """A new block object on this channel."""
        self._call("new_channel", channel)


def gps_l1_ca_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> GpsL1CaTelemetryDecoder:
    """GPS L1 C/A LNAV: 300-symbol subframes."""
    return GpsL1CaTelemetryDecoder(ctx, max_channels, max_rounds)


class CnavResult(NamedTuple):
    """One gnsship_cnav run: messages [max_channels, messages_per_run] (abi.CNAV_MESSAGE_DTYPE; slots k >= counts[c] are
    unspecified), counts int32[max_channels], faults uint8[max_channels], and the block's output stream per entry: tow_ms
    uint32[n_rounds, max_channels], sflags uint8[n_rounds, max_channels] (abi.CNAV_S_*), both 0 where the entry is no symbol."""
    messages: np.ndarray
    counts: np.ndarray
    faults: np.ndarray
    tow_ms: np.ndarray
    sflags: np.ndarray


class GpsCnavTelemetryDecoder(_TelemetryDecoder):
    """gps_l2c_telemetry_decoder_gs (signal abi.CNAV_L2C) or gps_l5_telemetry_decoder_gs (abi.CNAV_L5) up to the time of week
    for up to ``max_channels`` channels on the device, one block object per channel: libswiftcnav's two streaming Viterbi
    decoders, preamble rescan, CRC-24Q, the lock counter, and the block's watchdog, TOW stamp and valid_word
    (include/gnsship.h, gnsship_cnav_*).  max_rounds: the most entries per channel one run may carry."""
    _prefix, _result, _per_run = "gnsship_cnav", CnavResult, "messages_per_run"

    def __init__(self, ctx: Context, signal: int, max_channels: int, max_rounds: int):
        self.signal = int(signal)
        self._open(ctx, abi.CnavConf(max_rounds=int(max_rounds), signal=self.signal, reserved=0), max_channels, max_rounds)

    def _new_result(self, n_rounds: int):
        return CnavResult(np.zeros((self.max_channels, self.messages_per_run), abi.CNAV_MESSAGE_DTYPE),
                          np.zeros(self.max_channels, np.int32), np.zeros(self.max_channels, np.uint8),
                          np.zeros((n_rounds, self.max_channels), np.uint32), np.zeros((n_rounds, self.max_channels), np.uint8))

    def run_symbols(self, symbols, valid=None, out_valid=None, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """symbols float32[n_rounds, max_channels] (or a device pointer with on_device and n_rounds); valid and out_valid
        uint8 of the same shape (and place) or None.  Returns a CnavResult, or None when not host (asynchronous)."""
        return self._run_symbols(symbols, (("valid", valid), ("out_valid", out_valid)), on_device, n_rounds, host)

    def state(self, channel: int) -> np.ndarray:
        """Every member of the channel's block object: one abi.CNAV_STATE_DTYPE record (a 0-d array)."""
        st = np.zeros((), abi.CNAV_STATE_DTYPE)
        self._call("state_get", channel, ctypes.c_void_p(st.ctypes.data))
        return st

    def set_state(self, channel: int, state):
        """The channel's members become ``state`` (an abi.CNAV_STATE_DTYPE record, e.g. another handle's state())."""
        st = np.ascontiguousarray(state, abi.CNAV_STATE_DTYPE).reshape(())
        self._call("state_set", channel, ctypes.c_void_p(st.ctypes.data))

    def reset_channel(self, channel: int):
        """The block's reset()."""
        self._call("reset_channel", channel)

    def new_channel(self, channel: int):
        """A new block object on this channel."""
        self._call("new_channel", channel)


def gps_l2c_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> GpsCnavTelemetryDecoder:
    """GPS L2C CNAV (gps_l2c_telemetry_decoder_gs): 20 ms symbols, the TOW a double."""
    return GpsCnavTelemetryDecoder(ctx, abi.CNAV_L2C, max_channels, max_rounds)


def gps_l5_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> GpsCnavTelemetryDecoder:
    """GPS L5 CNAV (gps_l5_telemetry_decoder_gs): 10 ms symbols read from Prompt_Q, the TOW in integer milliseconds."""
    return GpsCnavTelemetryDecoder(ctx, abi.CNAV_L5, max_channels, max_rounds)


class DnavResult(NamedTuple):
    """One gnsship_dnav run: subframes [max_channels, subframes_per_run] (abi.DNAV_SUBFRAME_DTYPE; slots k >= counts[c] are
    unspecified), counts int32[max_channels], and the block's output stream per entry: tow_ms uint32[n_rounds, max_channels],
    sflags uint8[n_rounds, max_channels] (abi.DNAV_S_*), both 0 where the entry is no symbol."""
    subframes: np.ndarray
    counts: np.ndarray
    tow_ms: np.ndarray
    sflags: np.ndarray


class BeidouDnavTelemetryDecoder(_TelemetryDecoder):
    """beidou_b1i_telemetry_decoder_gs (signal abi.DNAV_B1I) or beidou_b3i_telemetry_decoder_gs (abi.DNAV_B3I) up to the time
    of week for up to ``channels`` channels on the device, one block object per channel: the 311-symbol history, preamble
    correlation, three-state frame sync, BCH(15,11,1) with its de-interleaver, the D1 / D2 FraID, Pnum and SOW, and the TOW
    stamp with valid_word (include/gnsship.h, gnsship_dnav_*).  max_rounds: the most entries per channel one run may carry."""
    _prefix, _result, _per_run, _state = "gnsship_dnav", DnavResult, "subframes_per_run", abi.DnavState

    def __init__(self, ctx: Context, channels: int, max_rounds: int, signal: int):
        self.signal = int(signal)
        self._open(ctx, abi.DnavConf(max_rounds=int(max_rounds), signal=self.signal, reserved=0), channels, max_rounds)

    def _new_result(self, n_rounds: int):
        return DnavResult(np.zeros((self.max_channels, self.subframes_per_run), abi.DNAV_SUBFRAME_DTYPE), np.zeros(self.max_channels, np.int32),
                          np.zeros((n_rounds, self.max_channels), np.uint32), np.zeros((n_rounds, self.max_channels), np.uint8))

    def run_symbols(self, symbols, valid=None, out_valid=None, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """symbols float32[n_rounds, max_channels] (or a device pointer with on_device and n_rounds); valid and out_valid
        uint8 of the same shape (and place) or None.  Returns a DnavResult, or None when not host (asynchronous)."""
        return self._run_symbols(symbols, (("valid", valid), ("out_valid", out_valid)), on_device, n_rounds, host)

    def reset_channel(self, channel: int):
        """The block's reset()."""
        self._call("reset_channel", channel)

    def set_satellite(self, channel: int, prn: int):
        """The block's set_satellite(): timing and decoder choice only."""
        self._call("set_satellite", channel, int(prn))

    def new_channel(self, channel: int, prn: int):
        """A new block object on this channel, constructed on this PRN."""
        self._call("new_channel", channel, int(prn))


def beidou_b1i_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> BeidouDnavTelemetryDecoder:
    """BeiDou B1I D1/D2 (beidou_b1i_telemetry_decoder_gs)."""
    return BeidouDnavTelemetryDecoder(ctx, max_channels, max_rounds, abi.DNAV_B1I)


def beidou_b3i_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> BeidouDnavTelemetryDecoder:
    """BeiDou B3I D1/D2 (beidou_b3i_telemetry_decoder_gs): a PRN above 58 takes the D1 decoder with the D2 timing."""
    return BeidouDnavTelemetryDecoder(ctx, max_channels, max_rounds, abi.DNAV_B3I)


class GnavResult(NamedTuple):
    """One gnsship_gnav run: strings [max_channels, strings_per_run] (abi.GNAV_STRING_DTYPE; slots k >= counts[c] are
    unspecified), counts int32[max_channels], and the block's output stream per entry: tow_ms uint32[n_rounds, max_channels],
    sflags uint8[n_rounds, max_channels] (abi.GNAV_S_*), both 0 where the entry is no symbol."""
    strings: np.ndarray
    counts: np.ndarray
    tow_ms: np.ndarray
    sflags: np.ndarray


class GlonassGnavTelemetryDecoder(_TelemetryDecoder):
    """glonass_l1_ca_telemetry_decoder_gs (signal abi.GNAV_L1CA) or glonass_l2_ca_telemetry_decoder_gs (abi.GNAV_L2CA) up to the
    time of week for up to ``channels`` channels on the device, one block object per channel: the 2000-symbol history, the
    time-mark correlation over its 300 oldest entries, three-state frame sync, the double half-bit sums, the Hamming check
    with its single-bit correction, what strings 1..5 give the time of week, glot_to_gpst and the double TOW stamp with
    valid_word (include/gnsship.h, gnsship_gnav_*).  max_rounds: the most entries per channel one run may carry."""
    _prefix, _result, _per_run = "gnsship_gnav", GnavResult, "strings_per_run"

    def __init__(self, ctx: Context, channels: int, max_rounds: int, signal: int):
        self.signal = int(signal)
        self._open(ctx, abi.GnavConf(max_rounds=int(max_rounds), signal=self.signal, reserved=0), channels, max_rounds)

    def _new_result(self, n_rounds: int):
        return GnavResult(np.zeros((self.max_channels, self.strings_per_run), abi.GNAV_STRING_DTYPE), np.zeros(self.max_channels, np.int32),
                          np.zeros((n_rounds, self.max_channels), np.uint32), np.zeros((n_rounds, self.max_channels), np.uint8))

    def run_symbols(self, symbols, valid=None, out_valid=None, on_device: bool = False, n_rounds: int = None, host: bool = True):
        """symbols float32[n_rounds, max_channels] (or a device pointer with on_device and n_rounds); valid and out_valid
        uint8 of the same shape (and place) or None (out_valid is accepted and not read, as in the blocks).  Returns a GnavResult, or None when not host (asynchronous)."""
        return self._run_symbols(symbols, (("valid", valid), ("out_valid", out_valid)), on_device, n_rounds, host)

    def state(self, channel: int) -> np.ndarray:
        """The channel's members (gnsship_gnav_state) as one abi.GNAV_STATE_DTYPE record."""
        st = np.zeros(1, abi.GNAV_STATE_DTYPE)
        self._call("state_get", channel, ctypes.c_void_p(st.ctypes.data))
        return st[0]

    def set_state(self, channel: int, st):
        """The channel's members become st (one abi.GNAV_STATE_DTYPE record)."""
        st = np.ascontiguousarray(np.asarray(st, abi.GNAV_STATE_DTYPE).reshape(1))
        self._call("state_set", channel, ctypes.c_void_p(st.ctypes.data))

    def set_satellite(self, channel: int, prn: int):
        """The block's set_satellite(): the PRN only."""
        self._call("set_satellite", channel, int(prn))

    def new_channel(self, channel: int, prn: int):
        """A new block object on this channel, constructed on this PRN."""
        self._call("new_channel", channel, int(prn))


def glonass_l1_ca_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> GlonassGnavTelemetryDecoder:
    """GLONASS L1 C/A GNAV (glonass_l1_ca_telemetry_decoder_gs)."""
    return GlonassGnavTelemetryDecoder(ctx, max_channels, max_rounds, abi.GNAV_L1CA)


def glonass_l2_ca_telemetry(ctx: Context, max_channels: int, max_rounds: int) -> GlonassGnavTelemetryDecoder:
    """GLONASS L2 C/A GNAV (glonass_l2_ca_telemetry_decoder_gs): the same algorithm."""
    return GlonassGnavTelemetryDecoder(ctx, max_channels, max_rounds, abi.GNAV_L2CA)


class DllPllVemlTracking(_Handle):
    """dll_pll_veml_tracking (dll_pll_veml_tracking.cc) for up to ``max_channels`` channels, the
    per-epoch loop resident on the device: ``start_tracking`` → :meth:`start`, ``general_work``
    over an IF buffer → :meth:`run` (one record per channel-epoch, TRK_EPOCH_DTYPE)."""
    _prefix = "gnsship_trk"

    def __init__(self, ctx: Context, conf: "abi.TrkConf", max_channels: int):
        self.ctx = ctx
        self.conf = conf
        self.max_channels = max_channels
        self._create(ctypes.byref(conf), max_channels)

    def start(self, channel: int, code_id: int, acq_delay_samples: float, acq_doppler_hz: float, acq_samplestamp: int,
              first_sample: int, data_code_id: int = -1, prn: int = 0):
        a = abi.TrkStartArgs(code_id=code_id, data_code_id=data_code_id, acq_delay_samples=acq_delay_samples,
                             acq_doppler_hz=acq_doppler_hz, acq_samplestamp_samples=acq_samplestamp, first_sample=first_sample,
                             prn=prn)
        self._call("start", channel, ctypes.byref(a))

    def start_many(self, starts):
        """gnsship_trk_start_many: `starts` = [(channel, code_id, acq_delay_samples, acq_doppler_hz,
        acq_samplestamp, first_sample[, data_code_id[, prn]]), ...] in one transaction."""
        n = len(starts)
        if n == 0:
            return
        chans = (ctypes.c_int32 * n)()
        args = (abi.TrkStartArgs * n)()
        for i, st in enumerate(starts):
            ch, code_id, delay, dop, stamp, first = st[:6]
            data_code_id = st[6] if len(st) > 6 else -1
            prn = st[7] if len(st) > 7 else 0
            chans[i] = ch
            args[i] = abi.TrkStartArgs(code_id=code_id, data_code_id=data_code_id, acq_delay_samples=delay, acq_doppler_hz=dop,
                                       acq_samplestamp_samples=stamp, first_sample=first, prn=prn)
        self._call("start_many", n, chans, args)

    def stop(self, channel: int):
        self._call("stop", channel)

    def telemetry_event(self, channel: int, tlm_event: int = 1):
        """msg_handler_telemetry_to_trk (dll_pll_veml_tracking.cc:617-640): event 1 = telemetry fault."""
        self._call("telemetry_event", channel, tlm_event)

    def channel_state(self, channel: int):
        st, nx = ctypes.c_int(), ctypes.c_uint64()
        self._call("channel_state", channel, ctypes.byref(st), ctypes.byref(nx))
        return st.value, nx.value

    def run(self, sig, buffer_first_sample: int, max_rounds: int, fmt: int = None, n_buffer_samples: int = None,
            records: bool = True, dump: bool = False):
        """sig: host ndarray or DeviceBuffer (pass fmt and n_buffer_samples).  Returns (records
        [max_rounds, max_channels] or None, rounds_done), plus the log_data dump records
        [max_rounds, max_channels] (TRK_DUMP_DTYPE; valid where the record has flags & 16) when dump."""
        out = np.zeros((max_rounds, self.max_channels), abi.TRK_EPOCH_DTYPE) if records else None
        dmp = np.zeros((max_rounds, self.max_channels), abi.TRK_DUMP_DTYPE) if dump else None
        if dump and not records:
            raise ValueError("dump records need the epoch records (flags & 16 marks them)")
        ptr, on_dev, f, n = _if_input(sig, fmt)
        if on_dev and n_buffer_samples is not None:
            n = n_buffer_samples
        done = ctypes.c_int()
        self._call("run_dump", ptr, f, on_dev, buffer_first_sample, n, max_rounds, out.ctypes.data if records else None,
                   dmp.ctypes.data if dump else None, ctypes.byref(done))
        return (out, done.value, dmp) if dump else (out, done.value)

    def run_ptr(self, dev_ptr: int, fmt: int, buffer_first_sample: int, n_buffer_samples: int, max_rounds: int) -> int:
        """general_work over a device IF buffer given as a raw pointer (e.g. a torch tensor's data_ptr,
        or an offset into one), no records: returns the rounds run."""
        done = ctypes.c_int()
        self._call("run_dump", ctypes.c_void_p(dev_ptr), fmt, 1, buffer_first_sample, n_buffer_samples, max_rounds, None, None, ctypes.byref(done))
        return done.value

    def launch_ptr(self, dev_ptr: int, fmt: int, buffer_first_sample: int, n_buffer_samples: int, max_rounds: int,
                   records: bool = False, dump: bool = False):
        """gnsship_trk_launch: enqueue the run on this engine's context stream and return at once
        (engines on other contexts of the same device run concurrently); :meth:`collect` waits."""
        self._call("launch", ctypes.c_void_p(dev_ptr), fmt, buffer_first_sample, n_buffer_samples, max_rounds, int(records), int(dump))
        self._pending = (max_rounds, records, dump)

    def collect(self, out: np.ndarray = None):
        """gnsship_trk_collect for the last launch_ptr: (records or None, rounds_done[, dump]).
        out: a caller's (max_rounds, max_channels) TRK_EPOCH_DTYPE array to fill (reused buffers)."""
        max_rounds, records, dump = self._pending
        if out is not None:
            if not records or out.dtype != abi.TRK_EPOCH_DTYPE or out.shape != (max_rounds, self.max_channels) or not out.flags.c_contiguous:
                raise ValueError("collect(out=): a C-contiguous (max_rounds, max_channels) TRK_EPOCH_DTYPE array, records launched")
        else:
            out = np.zeros((max_rounds, self.max_channels), abi.TRK_EPOCH_DTYPE) if records else None
        dmp = np.zeros((max_rounds, self.max_channels), abi.TRK_DUMP_DTYPE) if dump else None
        done = ctypes.c_int()
        self._call("collect", out.ctypes.data if records else None, dmp.ctypes.data if dump else None, ctypes.byref(done))
        return (out, done.value, dmp) if dump else (out, done.value)

    def set_trace(self, enable: bool = True):
        """gnsship_trk_set_trace: record every channel-epoch's correlator arguments and outputs."""
        self._call("set_trace", int(enable))

    def trace(self, max_rounds: int) -> np.ndarray:
        """The last run's trace, [max_rounds, max_channels] TRK_TRACE_DTYPE (max_rounds of that run)."""
        out = np.zeros((max_rounds, self.max_channels), abi.TRK_TRACE_DTYPE)
        self._call("trace_records", out.ctypes.data, out.size)
        return out

    def last_engine(self) -> int:
        """gnsship_trk_last_engine: the kernel the last run / launch ran (abi.TRK_ENGINE_*)."""
        v = ctypes.c_int(0)
        self._call("last_engine", ctypes.byref(v))
        return v.value

    def last_plan(self) -> dict:
        """gnsship_trk_last_plan: the variant the last run's launch function chose (abi.TrkPlan's members by name)."""
        p = abi.TrkPlan()
        self._call("last_plan", ctypes.byref(p))
        return p.as_dict()

    def states(self) -> np.ndarray:
        """Tracking state (0 idle/lost, 2, 3, 4) of every channel."""
        return np.array([self.channel_state(ch)[0] for ch in range(self.max_channels)], np.int32)

    @staticmethod
    def write_dump_files(prefix: str, records: np.ndarray, dumps: np.ndarray, append: bool = False, glonass: bool = False) -> list:
        """The reference's per-channel tracking dump files (<prefix><channel>.dat, dll_pll_veml_tracking.cc:
        set_channel :1674-1700, log_data :1376-1466): the records log_data wrote, in round order.
        glonass: the 88-byte record of glonass_l1_ca_dll_pll_tracking_cc (:641-701), which has no rate fields."""
        paths = []
        for ch in range(records.shape[1]):
            sel = (records[:, ch]["flags"] & abi.TRK_FLAG_DUMP) != 0
            path = f"{prefix}{ch}.dat"
            rows = np.ascontiguousarray(dumps[sel, ch])
            if glonass:
                short = np.zeros(len(rows), abi.TRK_DUMP_GLONASS_DTYPE)
                for name in abi.TRK_DUMP_GLONASS_DTYPE.names:
                    short[name] = rows[name]
                rows = short
            with open(path, "ab" if append else "wb") as f:
                f.write(rows.tobytes())
            paths.append(path)
        return paths
