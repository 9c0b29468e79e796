"""The Python surface of the five telemetry decoders (gnss_sim_receiver_amd.engine): class names, every public callable's
signature, the result tuples' fields and the factories, as literals.  The classes share one private base; what a caller
sees of each must not move with it.  Needs no GPU: the library loads without one."""
import inspect

import pytest

from gnss_sim_receiver_amd import engine

RUN_RECORDS = "(self, records, on_device: 'bool' = False, n_rounds: 'int' = None, host: 'bool' = True)"
RUN_TRK = '(self, trk: "\'DllPllVemlTracking\'", host: \'bool\' = True)'
RUN_SYMBOLS_OUT_VALID = "(self, symbols, valid=None, out_valid=None, on_device: 'bool' = False, n_rounds: 'int' = None, host: 'bool' = True)"
CHANNEL, CHANNEL_PRN = "(self, channel: 'int')", "(self, channel: 'int', prn: 'int')"
COMMON = {"__del__": "(self)", "close": "(self)", "outputs_device": "(self)", "run_records": RUN_RECORDS, "run_trk": RUN_TRK}

METHODS = {
    "GalileoTelemetryDecoder": {
        **COMMON,
        "__init__": "(self, ctx: 'Context', frame_type: 'int', max_channels: 'int', max_rounds: 'int', mode='reference')",
        "run_symbols": "(self, symbols, valid=None, on_device: 'bool' = False, n_rounds: 'int' = None, host: 'bool' = True)",
        "state": "(self, channel: 'int') -> 'dict'",
        "reset_channel": CHANNEL, "set_satellite": CHANNEL, "new_channel": CHANNEL},
    "GpsL1CaTelemetryDecoder": {
        **COMMON,
        "__init__": "(self, ctx: 'Context', max_channels: 'int', max_rounds: 'int')",
        "run_symbols": "(self, symbols, valid=None, flags180=None, on_device: 'bool' = False, n_rounds: 'int' = None, host: 'bool' = True)",
        "state": "(self, channel: 'int') -> 'dict'",
        "reset_channel": CHANNEL, "set_satellite": CHANNEL, "new_channel": CHANNEL},
    "GpsCnavTelemetryDecoder": {
        **COMMON,
        "__init__": "(self, ctx: 'Context', signal: 'int', max_channels: 'int', max_rounds: 'int')",
        "run_symbols": RUN_SYMBOLS_OUT_VALID,
        "state": "(self, channel: 'int') -> 'np.ndarray'", "set_state": "(self, channel: 'int', state)",
        "reset_channel": CHANNEL, "new_channel": CHANNEL},
    "BeidouDnavTelemetryDecoder": {
        **COMMON,
        "__init__": "(self, ctx: 'Context', channels: 'int', max_rounds: 'int', signal: 'int')",
        "run_symbols": RUN_SYMBOLS_OUT_VALID,
        "state": "(self, channel: 'int') -> 'dict'",
        "reset_channel": CHANNEL, "set_satellite": CHANNEL_PRN, "new_channel": CHANNEL_PRN},
    "GlonassGnavTelemetryDecoder": {
        **COMMON,
        "__init__": "(self, ctx: 'Context', channels: 'int', max_rounds: 'int', signal: 'int')",
        "run_symbols": RUN_SYMBOLS_OUT_VALID,
        "state": "(self, channel: 'int') -> 'np.ndarray'", "set_state": "(self, channel: 'int', st)",
        "set_satellite": CHANNEL_PRN, "new_channel": CHANNEL_PRN},
}
ABSENT = {"GalileoTelemetryDecoder": ["set_state"], "GpsL1CaTelemetryDecoder": ["set_state"], "GpsCnavTelemetryDecoder": ["set_satellite"],
          "BeidouDnavTelemetryDecoder": ["set_state"], "GlonassGnavTelemetryDecoder": ["reset_channel"]}

FIELDS = {"TlmResult": ("pages", "bits", "counts", "faults"),
          "LnavResult": ("subframes", "counts", "faults", "tow_ms", "sflags"),
          "CnavResult": ("messages", "counts", "faults", "tow_ms", "sflags"),
          "DnavResult": ("subframes", "counts", "tow_ms", "sflags"),
          "GnavResult": ("strings", "counts", "tow_ms", "sflags")}

PLAIN, WITH_MODE = "(ctx: 'Context', max_channels: 'int', max_rounds: 'int')", "(ctx: 'Context', max_channels: 'int', max_rounds: 'int', mode='reference')"
FACTORIES = {"galileo_inav_telemetry": (WITH_MODE, "GalileoTelemetryDecoder"), "galileo_fnav_telemetry": (WITH_MODE, "GalileoTelemetryDecoder"),
             "galileo_cnav_telemetry": (WITH_MODE, "GalileoTelemetryDecoder"), "gps_l1_ca_telemetry": (PLAIN, "GpsL1CaTelemetryDecoder"),
             "gps_l2c_telemetry": (PLAIN, "GpsCnavTelemetryDecoder"), "gps_l5_telemetry": (PLAIN, "GpsCnavTelemetryDecoder"),
             "beidou_b1i_telemetry": (PLAIN, "BeidouDnavTelemetryDecoder"), "beidou_b3i_telemetry": (PLAIN, "BeidouDnavTelemetryDecoder"),
             "glonass_l1_ca_telemetry": (PLAIN, "GlonassGnavTelemetryDecoder"), "glonass_l2_ca_telemetry": (PLAIN, "GlonassGnavTelemetryDecoder")}


def public_callables(cls):
    return {n for n in dir(cls) if callable(getattr(cls, n)) and (not n.startswith("_") or n in ("__init__", "__del__"))}


@pytest.mark.parametrize("name", list(METHODS))
def test_class_methods_and_signatures(name):
    cls = getattr(engine, name)
    assert cls.__name__ == name and cls.__doc__
    assert public_callables(cls) == set(METHODS[name])
    for method, sig in METHODS[name].items():
        assert str(inspect.signature(getattr(cls, method))) == sig, (name, method)
        assert method in ("__init__", "__del__", "close") or getattr(cls, method).__doc__, (name, method)
    for method in ABSENT[name]:
        assert not hasattr(cls, method), (name, method)


@pytest.mark.parametrize("name", list(FIELDS))
def test_result_tuples(name):
    cls = getattr(engine, name)
    assert cls._fields == FIELDS[name] and issubclass(cls, tuple) and cls.__doc__
    assert str(inspect.signature(cls)) == "(" + ", ".join(f"{f}: ForwardRef('np.ndarray')" for f in FIELDS[name]) + ")"


def test_factories():
    assert {n for n in dir(engine) if n.endswith("_telemetry")} == set(FACTORIES)
    for name, (args, returns) in FACTORIES.items():
        fn = getattr(engine, name)
        assert str(inspect.signature(fn)) == f"{args} -> '{returns}'" and fn.__doc__, name
