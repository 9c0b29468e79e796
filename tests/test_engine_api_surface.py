"""The Python surface of gnss_sim_receiver_amd.engine outside the telemetry decoders (tests/test_tlm_api_surface.py holds
those): every public class with its public callables, properties and class attributes, every public function, their
signatures, and which of them carry a docstring, as literals.  The handle classes share one private base; what a caller
sees of each must not move with it.  Needs no GPU: the library loads without one."""
import inspect

import pytest

from gnss_sim_receiver_amd import engine

TELEMETRY = {"GalileoTelemetryDecoder", "GpsL1CaTelemetryDecoder", "GpsCnavTelemetryDecoder", "BeidouDnavTelemetryDecoder",
             "GlonassGnavTelemetryDecoder", "TlmResult", "LnavResult", "CnavResult", "DnavResult", "GnavResult"}
DUNDER = ("__init__", "__del__", "__enter__", "__exit__")

# name -> signature, "property" or "attribute"
CLASSES = {'Context': {'__del__': '(self)',
             '__enter__': '(self)',
             '__exit__': '(self, *a)',
             '__init__': "(self, device: 'int' = 0)",
             'close': '(self)',
             'event_elapsed_ms': "(self, a: 'int', b: 'int') -> 'float'",
             'event_record': "(self, slot: 'int')",
             'set_code': "(self, code_id: 'int', code: 'np.ndarray')",
             'stream': "(self) -> 'int'",
             'sync': '(self)',
             'upload': '(self, host: \'np.ndarray\') -> "\'DeviceBuffer\'"'},
 'DeviceBuffer': {'__del__': '(self)',
                  '__init__': "(self, ctx: 'Context', nbytes: 'int')",
                  'download': "(self, out: 'np.ndarray', offset: 'int' = 0)",
                  'free': '(self)',
                  'upload': "(self, host: 'np.ndarray', offset: 'int' = 0)",
                  'wrap': '(ctx: \'Context\', ptr: \'int\', nbytes: \'int\') -> "\'DeviceBuffer\'"'},
 'Comm': {'__init__': "(self, ctx: 'Context', n_ranks: 'int', rank: 'int', uid: 'bytes')",
          'allgather': "(self, dev_send: 'int', dev_recv: 'int', bytes_per_rank: 'int')",
          'broadcast': "(self, dev_ptr: 'int', nbytes: 'int', root: 'int' = 0)",
          'close': '(self)',
          'from_process_group': "(ctx: 'Context')",
          'max_f64': "(self, values) -> 'np.ndarray'"},
 'MultiCorrelatorRealCodes': {'Carrier_wipeoff_multicorrelator_resampler': '(self, rem_carrier_phase_in_rad, phase_step_rad, phase_rate_step_rad, '
                                                                           'rem_code_phase_chips, code_phase_step_chips, code_phase_rate_step_chips, '
                                                                           "signal_length_samples) -> 'bool'",
                              '__del__': '(self)',
                              'close': '(self)',  # new with the shared base; free() stays, and returns True
                              '__init__': "(self, ctx: 'Context', rotator: 'int' = -1)",
                              'free': "(self) -> 'bool'",
                              'init': "(self, max_signal_length_samples: 'int', n_correlators: 'int') -> 'bool'",
                              'set_high_dynamics_resampler': "(self, use: 'bool')",
                              'set_input_output_vectors': "(self, corr_out: 'np.ndarray', sig_in: 'np.ndarray') -> 'bool'",
                              'set_local_code_and_taps': "(self, code_length_chips: 'int', local_code_in: 'np.ndarray', shifts_chips: 'np.ndarray') "
                                                         "-> 'bool'"},
 'CorrelatorBatch': {'__del__': '(self)',
                     '__init__': "(self, ctx: 'Context', max_jobs: 'int')",
                     'close': '(self)',
                     'launch': "(self, samples: 'DeviceBuffer', fmt: 'int' = 0)",
                     'launch_pipelined': '(self, dev_ptr: \'int\', fmt: \'int\' = 0, next_batch: "\'CorrelatorBatch\'" = None, next2: '
                                         '"\'CorrelatorBatch\'" = None)',
                     'launch_ptr': "(self, dev_ptr: 'int', fmt: 'int' = 0, stages: 'int' = 3)",
                     'results': "(self) -> 'np.ndarray'",
                     'set_jobs': "(self, jobs: 'np.ndarray', n_buffer_samples: 'int')"},
 'PcpsAcquisition': {'__del__': '(self)',
                     '__init__': "(self, ctx: 'Context', fs_in: 'int', fft_size: 'int', doppler_max: 'int', doppler_step: 'int', doppler_center: "
                                 "'int' = 0, use_cfar: 'bool' = True, samples_per_chip: 'int' = None, samples_per_code: 'float' = None, max_prns: "
                                 "'int' = 1, max_dwells: 'int' = 1, chip_rate: 'float' = 1023000.0, ms_per_code: 'int' = 1, consumed_samples: 'int' "
                                 "= 0, bit_transition_flag: 'bool' = False, resampler_ratio: 'float' = 1.0, resampler_latency_samples: 'int' = 0)",
                     'close': '(self)',
                     'layout': 'property',
                     'run': "(self, sig, n_prns: 'int' = 1, want_grid: 'bool' = False, fmt: 'int' = None)",
                     'run_fdma': "(self, sig, prn_slot: 'int' = 0, want_grid: 'bool' = False, fmt: 'int' = None)",
                     'set_grid': "(self, doppler_max: 'int', doppler_step: 'int', doppler_center: 'int' = 0)",
                     'set_grid_fdma': "(self, doppler_max: 'int', doppler_step: 'int', doppler_center: 'int', bias_hz)",
                     'set_grid_step2': "(self, doppler_center_step_two: 'float', doppler_step2: 'float', num_doppler_bins_step2: 'int', "
                                       "step_one_input_power: 'float')",
                     'set_local_code': "(self, code: 'np.ndarray', prn_slot: 'int' = 0)"},
 'AcqResampler': {'__del__': '(self)',  # new with the shared base: the handle is released when it is collected
                  '__init__': "(self, ctx: 'Context', taps: 'np.ndarray', decimation: 'int', max_in_samples: 'int')",
                  'close': '(self)',
                  'latency': 'property',
                  'reset': '(self)',
                  'run': "(self, x, fmt: 'int' = None, on_device: 'bool' = False, n_in: 'int' = None)"},
 'SignalConditioner': {'__del__': '(self)',
                       '__init__': "(self, ctx: 'Context', fs_in: 'float', bands, max_in_samples: 'int')",
                       'close': '(self)',
                       'n_bands': 'property',
                       'reset': "(self, first_sample: 'int' = 0)",
                       'run': "(self, x, fmt: 'int' = None, on_device: 'bool' = False, n_in: 'int' = None, dev_dst=None, host: 'bool' = None)",
                       'samples_in': "(self) -> 'int'"},
 'InterferenceMitigation': {'FORMS': 'attribute',
                            'KINDS': 'attribute',
                            '__del__': '(self)',
                            '__init__': "(self, ctx: 'Context', kind, max_in_samples: 'int', pfa: 'float' = None, threshold: 'float' = 0.0, "
                                        "p_c_factor: 'float' = 0.9, length: 'int' = 32, n_segments_est: 'int' = 12500, n_segments_reset: 'int' = "
                                        "5000000, n_segments_coeff: 'int' = 1, chain_form='auto')",
                            'close': '(self)',
                            'reset': '(self)',
                            'run': "(self, x, on_device: 'bool' = False, n_in: 'int' = None, dev_dst=None, host: 'bool' = None)",
                            'state': "(self) -> 'dict'"},
 'ViterbiDecoder': {'MODES': 'attribute',
                    '__del__': '(self)',
                    '__init__': "(self, ctx: 'Context', max_channels: 'int', data_length: 'int', interleaver_rows: 'int' = 0, interleaver_cols: "
                                "'int' = 0, invert_g2: 'bool' = False, mode='reference', g=(121, 91), constraint_length: 'int' = 7, rate_n: 'int' = "
                                '2)',
                    'close': '(self)',
                    'reset_channel': "(self, channel: 'int')",
                    'run': "(self, symbols, channels, negate=None, on_device: 'bool' = False, n_frames: 'int' = None, bits_dev=None, host: 'bool' = "
                           'True)',
                    'state': "(self, channel: 'int') -> 'np.ndarray'"},
 'DllPllVemlTracking': {'__del__': '(self)',
                        '__init__': '(self, ctx: \'Context\', conf: "\'abi.TrkConf\'", max_channels: \'int\')',
                        'channel_state': "(self, channel: 'int')",
                        'close': '(self)',
                        'collect': "(self, out: 'np.ndarray' = None)",
                        'last_engine': "(self) -> 'int'",
                        'last_plan': "(self) -> 'dict'",
                        'launch_ptr': "(self, dev_ptr: 'int', fmt: 'int', buffer_first_sample: 'int', n_buffer_samples: 'int', max_rounds: 'int', "
                                      "records: 'bool' = False, dump: 'bool' = False)",
                        'run': "(self, sig, buffer_first_sample: 'int', max_rounds: 'int', fmt: 'int' = None, n_buffer_samples: 'int' = None, "
                               "records: 'bool' = True, dump: 'bool' = False)",
                        'run_ptr': "(self, dev_ptr: 'int', fmt: 'int', buffer_first_sample: 'int', n_buffer_samples: 'int', max_rounds: 'int') -> "
                                   "'int'",
                        'set_trace': "(self, enable: 'bool' = True)",
                        'start': "(self, channel: 'int', code_id: 'int', acq_delay_samples: 'float', acq_doppler_hz: 'float', acq_samplestamp: "
                                 "'int', first_sample: 'int', data_code_id: 'int' = -1, prn: 'int' = 0)",
                        'start_many': '(self, starts)',
                        'states': "(self) -> 'np.ndarray'",
                        'stop': "(self, channel: 'int')",
                        'telemetry_event': "(self, channel: 'int', tlm_event: 'int' = 1)",
                        'trace': "(self, max_rounds: 'int') -> 'np.ndarray'",
                        'write_dump_files': "(prefix: 'str', records: 'np.ndarray', dumps: 'np.ndarray', append: 'bool' = False, glonass: 'bool' = "
                                            "False) -> 'list'"}}

FUNCTIONS = {'sample_format': "(x: 'np.ndarray') -> 'int'",
 'device_count': "() -> 'int'",
 'comm_unique_id': "() -> 'bytes'",
 'correlate_host': "(ctx: 'Context', samples: 'np.ndarray', jobs: 'np.ndarray', codes: 'list') -> 'np.ndarray'",
 'glonass_l1_ca_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', freq_channels=range(-7, 7), sampled_ms: "
                                   "'int' = 1, **kw) -> 'PcpsAcquisition'",
 'glonass_l2_ca_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', freq_channels=range(-7, 7), sampled_ms: "
                                   "'int' = 1, **kw) -> 'PcpsAcquisition'",
 'glonass_l1_ca_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'glonass_l2_ca_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'gps_l5i_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', sampled_ms: 'int' = 1, **kw) -> "
                             "'PcpsAcquisition'",
 'gps_l5_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'beidou_b3i_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', sampled_ms: 'int' = 1, **kw) -> "
                                "'PcpsAcquisition'",
 'gps_l2_m_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', sampled_ms: 'int' = 20, **kw) -> "
                              "'PcpsAcquisition'",
 'beidou_b3i_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'gps_l2c_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'galileo_e5a_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', sampled_ms: 'int' = 1, acquire_pilot: "
                                 "'bool' = False, acquire_iq: 'bool' = False, **kw) -> 'PcpsAcquisition'",
 'galileo_e5b_pcps_acquisition': "(ctx: 'Context', fs_in: 'int', doppler_max: 'int', doppler_step: 'int', sampled_ms: 'int' = 1, acquire_pilot: "
                                 "'bool' = False, acquire_iq: 'bool' = False, **kw) -> 'PcpsAcquisition'",
 'galileo_e5a_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'galileo_e5b_trk_conf': '(fs_in: \'float\', **kw) -> "\'abi.TrkConf\'"',
 'firdes_low_pass': "(lib, gain: 'float', fs: 'float', cutoff: 'float', transition: 'float') -> 'np.ndarray'",
 'acq_resampler_design': "(lib, fs_in: 'int', opt_acq_fs: 'float')",
 'cond_lowpass_taps': "(lib, fs: 'float', decimation: 'int', bw: 'float' = 0.0, tw: 'float' = 0.0) -> 'np.ndarray'",
 'mit_threshold': "(lib, pfa: 'float', length: 'int') -> 'float'",
 'galileo_inav_page_decoder': "(ctx: 'Context', max_channels: 'int', mode='reference') -> 'ViterbiDecoder'",
 'galileo_fnav_page_decoder': "(ctx: 'Context', max_channels: 'int', mode='reference') -> 'ViterbiDecoder'",
 'galileo_cnav_page_decoder': "(ctx: 'Context', max_channels: 'int', mode='reference') -> 'ViterbiDecoder'"}

DOCUMENTED = ['sample_format', 'DeviceBuffer.wrap', 'comm_unique_id', 'Comm.from_process_group', 'Comm.max_f64', 'CorrelatorBatch.launch_pipelined',
 'correlate_host', 'PcpsAcquisition.layout', 'PcpsAcquisition.run', 'PcpsAcquisition.run_fdma', 'PcpsAcquisition.set_grid_fdma',
 'PcpsAcquisition.set_grid_step2', 'glonass_l1_ca_pcps_acquisition', 'glonass_l2_ca_pcps_acquisition', 'glonass_l1_ca_trk_conf',
 'glonass_l2_ca_trk_conf', 'gps_l5i_pcps_acquisition', 'gps_l5_trk_conf', 'beidou_b3i_pcps_acquisition', 'gps_l2_m_pcps_acquisition',
 'beidou_b3i_trk_conf', 'gps_l2c_trk_conf', 'galileo_e5a_pcps_acquisition', 'galileo_e5b_pcps_acquisition', 'galileo_e5a_trk_conf',
 'galileo_e5b_trk_conf', 'firdes_low_pass', 'acq_resampler_design', 'AcqResampler.run', 'cond_lowpass_taps', 'SignalConditioner.run', 'mit_threshold',
 'InterferenceMitigation.run', 'ViterbiDecoder.reset_channel', 'ViterbiDecoder.run', 'ViterbiDecoder.state', 'galileo_inav_page_decoder',
 'galileo_fnav_page_decoder', 'galileo_cnav_page_decoder', 'DllPllVemlTracking.collect', 'DllPllVemlTracking.last_engine',
 'DllPllVemlTracking.last_plan', 'DllPllVemlTracking.launch_ptr', 'DllPllVemlTracking.run', 'DllPllVemlTracking.run_ptr',
 'DllPllVemlTracking.set_trace', 'DllPllVemlTracking.start_many', 'DllPllVemlTracking.states', 'DllPllVemlTracking.telemetry_event',
 'DllPllVemlTracking.trace', 'DllPllVemlTracking.write_dump_files']


def own(name, obj):
    return not name.startswith("_") and getattr(obj, "__module__", None) == engine.__name__ and name not in TELEMETRY and \
        not name.endswith("_telemetry")


def members(cls):
    """The class's public names and the four special methods it or a base of it defines."""
    out = {}
    for n in dir(cls):
        if n.startswith("_") and (n not in DUNDER or all(n not in vars(b) for b in cls.__mro__[:-1])):
            continue
        a = inspect.getattr_static(cls, n)
        out[n] = "property" if isinstance(a, property) else str(inspect.signature(getattr(cls, n))) if callable(getattr(cls, n)) else "attribute"
    return out


def test_the_module_has_these_public_names_and_no_others():
    classes = {n for n, o in vars(engine).items() if own(n, o) and inspect.isclass(o) and not issubclass(o, tuple)}
    functions = {n for n, o in vars(engine).items() if own(n, o) and inspect.isfunction(o)}
    assert classes == set(CLASSES) and functions == set(FUNCTIONS)
    assert engine.AcqLayout._fields == ("kind", "P", "row_len", "radix", "ct_rows") and engine.AcqLayout.__doc__
    assert (engine.GALILEO_INAV_PAGE, engine.GALILEO_FNAV_PAGE, engine.GALILEO_CNAV_PAGE) == ((8, 30, 114), (8, 61, 238), (8, 123, 486))


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_members_and_signatures(name):
    cls = getattr(engine, name)
    assert cls.__name__ == name and cls.__doc__
    assert members(cls) == CLASSES[name]


@pytest.mark.parametrize("name", list(FUNCTIONS))
def test_function_signatures(name):
    assert str(inspect.signature(getattr(engine, name))) == FUNCTIONS[name]


def test_docstrings_stay():
    for path in DOCUMENTED:
        obj = engine
        for part in path.split("."):
            obj = inspect.getattr_static(obj, part) if inspect.isclass(obj) else getattr(obj, part)
        obj = obj.fget if isinstance(obj, property) else getattr(obj, "__func__", obj)
        assert obj.__doc__, path


def test_class_attributes():
    from gnss_sim_receiver_amd import abi
    assert engine.InterferenceMitigation.KINDS == {"pulse-blanking": abi.MIT_PULSE_BLANKING, "notch": abi.MIT_NOTCH, "notch-lite": abi.MIT_NOTCH_LITE}
    assert engine.InterferenceMitigation.FORMS == {"auto": abi.MIT_CHAIN_AUTO, "serial": abi.MIT_CHAIN_SERIAL, "speculative": abi.MIT_CHAIN_SPECULATIVE}
    assert engine.ViterbiDecoder.MODES == {"reference": abi.VIT_MODE_REFERENCE, "full": abi.VIT_MODE_FULL}
    assert not hasattr(engine.Comm, "__del__")  # destroying a communicator is a collective: never from the garbage collector
