"""ctypes binding of libacarsdec_amd.so (include/acarsdec_amd.h) -- the same stub a cffi/ctypes
host would write against the C ABI.  No compute happens in Python."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# ACARSDEC_AMD_LIB: measurement aid (A/B timing of two builds on one box, the stamp build); the product is the in-tree path
LIB_PATH = os.environ.get("ACARSDEC_AMD_LIB") or os.path.join(HERE, "lib", "libacarsdec_amd.so")
# the lab build: every measurement kernel variant and debug shape; tests and probes only (Decoder(lab=True), tune(..., lab=True))
LAB_PATH = os.path.join(HERE, "lib", "libacarsdec_amd_lab.so")

OK, EINVAL, ENOMEM, EHIP, ENODEV, EOVERFLOW, ESTATE, EAGAIN = 0, -1, -2, -3, -4, -5, -6, -7
F_BITLOG, F_TIMING, F_REPAIR, F_EXACT_FIR, F_PRECISE_MIXER = 1, 2, 4, 8, 16
INTRATE, BLOCK, MAXDECIM, FLEN, TXTMAX = 12500, 1024, 320, 11, 250
MAXDECIM_SAMPLES = 1024
FMT_CS16, FMT_S16_SPLIT, FMT_F32_REAL = 1, 2, 3
FMT_CS8, FMT_CF32 = 4, 5                   # SigMF ci8 / cf32_le
FMT_CU8 = 6                                # rtl_sdr files, SigMF cu8: on the rate entry points only
# acg_lab_samples_launch.family
FIR_STREAMING, FIR_WORKGROUP, FIR_MATRIX, FIR_SHARED_VECTOR = 1, 2, 3, 4
PCM_S16, PCM_F32 = 1, 2


class Config(C.Structure):
    _fields_ = [("device", C.c_int), ("nch", C.c_int), ("nstreams", C.c_int), ("decim", C.c_int),
                ("ntaps", C.c_int), ("max_blocks", C.c_int), ("flags", C.c_uint32), ("max_lag", C.c_int)]


class ChanState(C.Structure):
    _fields_ = [("MskPhi", C.c_double), ("MskDf", C.c_double), ("MskLvlSum", C.c_double),
                ("MskClk", C.c_float), ("MskBitCount", C.c_int), ("MskS", C.c_uint), ("idx", C.c_uint),
                ("inb", C.c_float * (2 * FLEN)), ("outbits", C.c_int), ("nbits", C.c_int),
                ("Acarsstate", C.c_int), ("blk_len", C.c_int), ("blk_err", C.c_int), ("soh_back", C.c_int)]


class Frame(C.Structure):
    _fields_ = [("chn", C.c_int), ("len", C.c_int), ("err", C.c_int), ("lvl", C.c_float),
                ("crc", C.c_ubyte * 2), ("txt", C.c_ubyte * TXTMAX),
                ("end_bit", C.c_longlong), ("end_sample", C.c_longlong), ("soh_sample", C.c_longlong)]


class Msg(C.Structure):
    """acg_msg: outputmsg()'s field split as a fixed binary record"""
    _fields_ = [("chn", C.c_int), ("err", C.c_int), ("lvl", C.c_float), ("txt_len", C.c_int),
                ("end_bit", C.c_longlong), ("end_sample", C.c_longlong), ("soh_sample", C.c_longlong), ("reserved1", C.c_int),
                ("reserved2", C.c_char), ("mode", C.c_char), ("addr", C.c_char * 8), ("ack", C.c_char), ("label", C.c_char * 3),
                ("bid", C.c_char), ("no", C.c_char * 5), ("fid", C.c_char * 7), ("bs", C.c_char), ("be", C.c_char),
                ("down", C.c_char), ("txt", C.c_ubyte * 242), ("reserved3", C.c_int)]


MSGF_DOWNLINK_ONLY, MSGF_SKIP_EMPTY, MSGF_MAXLABELS = 1, 2, 64


class MsgFilter(C.Structure):
    """acg_msg_filter: the CLI's -A / -e flags and -b label list"""
    _fields_ = [("flags", C.c_uint32), ("nlabels", C.c_int), ("labels", (C.c_char * 4) * MSGF_MAXLABELS)]


class Oooi(C.Structure):
    """acg_oooi: label.c's oooi_t (acarsdec.h:94-102) and DecodeLabel()'s return value"""
    _fields_ = [("da", C.c_char * 5), ("sa", C.c_char * 5), ("eta", C.c_char * 5), ("gout", C.c_char * 5), ("gin", C.c_char * 5),
                ("woff", C.c_char * 5), ("won", C.c_char * 5), ("decoded", C.c_char), ("reserved", C.c_char * 4)]


class FlightConfig(C.Structure):
    """acg_flight_config: t0 of the sample clock, the CLI's -t, the table's capacity"""
    _fields_ = [("t0_sec", C.c_longlong), ("t0_usec", C.c_int), ("mdly", C.c_int), ("max_flights", C.c_int)]


class Flight(C.Structure):
    """acg_flight: one entry of the flight table (flight_t, output.c:345-358)"""
    _fields_ = [("addr", C.c_char * 8), ("fid", C.c_char * 7), ("rt", C.c_ubyte), ("nbm", C.c_int), ("first_chn", C.c_int),
                ("last_chn", C.c_int), ("reserved1", C.c_int), ("chm", C.c_ulonglong), ("ts_sample", C.c_longlong),
                ("tl_sample", C.c_longlong), ("ts_sec", C.c_longlong), ("tl_sec", C.c_longlong), ("ts_usec", C.c_int),
                ("tl_usec", C.c_int), ("da", C.c_char * 5), ("sa", C.c_char * 5), ("eta", C.c_char * 5), ("gout", C.c_char * 5),
                ("gin", C.c_char * 5), ("woff", C.c_char * 5), ("won", C.c_char * 5), ("reserved2", C.c_char * 5)]


class Route(C.Structure):
    """acg_route: one route record (routejson(), output.c:428-456)"""
    _fields_ = [("soh_sample", C.c_longlong), ("sec", C.c_longlong), ("usec", C.c_int), ("chn", C.c_int), ("fid", C.c_char * 7),
                ("sa", C.c_char * 5), ("da", C.c_char * 5), ("addr", C.c_char * 8), ("reserved", C.c_char * 7)]


class FlightEvent(C.Structure):
    """acg_flight_event: one message that reaches addFlight(), as it travels from a peer context to the owner of the table"""
    _fields_ = [("end_sample", C.c_longlong), ("soh_sample", C.c_longlong), ("sec", C.c_longlong), ("usec", C.c_int), ("chn", C.c_int),
                ("addr", C.c_char * 8), ("fid", C.c_char * 7), ("e_ok", C.c_ubyte), ("oooi", Oooi)]


# the same record as a numpy structured dtype (Decoder.drain_flight_events hands out arrays of it); oooi: its 40 bytes
FLIGHT_EVENT_DTYPE = [("end_sample", "<i8"), ("soh_sample", "<i8"), ("sec", "<i8"), ("usec", "<i4"), ("chn", "<i4"), ("addr", "S8"),
                      ("fid", "S7"), ("e_ok", "u1"), ("oooi", "V40")]


class ReasmConfig(C.Structure):
    """acg_reasm_config: t0 of the sample clock, the table's capacity (0 = 1024 chains), the longest text (0 = 3584 bytes)"""
    _fields_ = [("t0_sec", C.c_longlong), ("t0_usec", C.c_int), ("max_msgs", C.c_int), ("max_text", C.c_int)]


class ReasmMsg(C.Structure):
    """acg_reasm_msg: one completed multi-block message; its text lies at text_off of the same call's text buffer"""
    _fields_ = [("chn", C.c_int), ("nfrag", C.c_int), ("end_bit", C.c_longlong), ("end_sample", C.c_longlong), ("soh_sample", C.c_longlong),
                ("first_soh_sample", C.c_longlong), ("text_off", C.c_ulonglong), ("text_len", C.c_uint), ("down", C.c_char),
                ("addr", C.c_char * 8), ("label", C.c_char * 3), ("msn", C.c_char * 4), ("reserved", C.c_char * 12)]


REASM_UNKNOWN, REASM_COMPLETE, REASM_IN_PROGRESS, REASM_SKIPPED, REASM_DUPLICATE, REASM_OUT_OF_SEQUENCE, REASM_ARGS_INVALID, REASM_OVERFLOW = range(8)
# the same record as a numpy structured dtype (Decoder.drain_reassembled hands out arrays of it)
REASM_MSG_DTYPE = [("chn", "<i4"), ("nfrag", "<i4"), ("end_bit", "<i8"), ("end_sample", "<i8"), ("soh_sample", "<i8"), ("first_soh_sample", "<i8"),
                   ("text_off", "<u8"), ("text_len", "<u4"), ("down", "u1"), ("addr", "S8"), ("label", "S3"), ("msn", "S4"), ("reserved", "V12")]


class FlightTextConfig(C.Structure):
    """acg_flight_text_config: the monitor's mask columns (the reference's nbch) and the route line's station id"""
    _fields_ = [("nbch", C.c_int), ("station_id", C.c_char * 33)]


class ChanStats(C.Structure):
    """acg_chan_stats: one channel's reception statistics (the events the reference reports under -v)"""
    _fields_ = [(n, C.c_uint) for n in ("blocks", "too_short", "parity_many", "parity_blocks", "parity_errs", "crc_errors", "unfixable",
                                        "fixed", "parity_problem", "kept", "miss_txt_end", "uplink_dropped", "label_dropped",
                                        "empty_dropped", "delivered", "reserved")] + \
               [("lvl_min", C.c_double), ("lvl_max", C.c_double), ("last_end_sample", C.c_longlong)]


# the same record as a numpy structured dtype (Decoder.stats hands out arrays of it)
CHAN_STATS_DTYPE = [(n, "<u4") for n, _ in ChanStats._fields_[:16]] + [("lvl_min", "<f8"), ("lvl_max", "<f8"), ("last_end_sample", "<i8")]


MONITOR_CLS_LEN, MONITOR_HDR_LEN, MONITOR_ROW_MAX, ROUTE_LINE_MAX = 7, 110, 78, 363
JSON_LINE_MAX = 2496


TEXT_REC_MAX = 704
TEXT_ONELINE, TEXT_STD, TEXT_PP, TEXT_SV = 1, 2, 3, 4
TEXT_F_DATE, TEXT_F_FREQ = 1, 2
SINK_JSON, SINK_TEXT = 1, 2             # acg_sink_keys
SINK_KEY_END_BITS = 44                   # a key is (channel number handed out) << 44 | end_bit


class TextConfig(C.Structure):
    """acg_text_config: the format (printoneline / printmsg / Netoutpp / Netoutsv), its flags, t0 of the sample clock, the station id"""
    _fields_ = [("format", C.c_int), ("flags", C.c_uint), ("t0_sec", C.c_longlong), ("t0_usec", C.c_int), ("station_id", C.c_char * 33)]


class JsonConfig(C.Structure):
    """acg_json_config: t0 of the sample clock, the station id (-i) and the "app" object of every JSON line"""
    _fields_ = [("t0_sec", C.c_longlong), ("t0_usec", C.c_int), ("station_id", C.c_char * 33), ("app_name", C.c_char * 17),
                ("app_ver", C.c_char * 17)]


OUT_MSGS, OUT_JSON, OUT_LEGS_MAX = 0x10, 0x20, 4      # acg_out_leg.kind beside TEXT_*; SINK_OUTPUTS: acg_sink_keys
SINK_OUTPUTS = 4


class OutLeg(C.Structure):
    """acg_out_leg: OUT_MSGS, OUT_JSON or a TEXT_* format, and the TEXT_F_* flags that format takes"""
    _fields_ = [("kind", C.c_int), ("flags", C.c_uint)]


class OutputsConfig(C.Structure):
    """acg_outputs_config: the legs rendered from one take, one t0 and one station / app for all of them"""
    _fields_ = [("nlegs", C.c_int), ("leg", OutLeg * OUT_LEGS_MAX), ("t0_sec", C.c_longlong), ("t0_usec", C.c_int), ("station_id", C.c_char * 33),
                ("app_name", C.c_char * 17), ("app_ver", C.c_char * 17)]


class OutBuf(C.Structure):
    """acg_out_buf: one leg's buffers in an outputs call"""
    _fields_ = [("out", C.c_void_p), ("cap", C.c_size_t), ("offs", C.c_void_p), ("oooi", C.c_void_p), ("nbytes", C.c_size_t)]


class LaunchShape(C.Structure):
    """acg_lab_launch_shape: the down-converter launch the library makes for one launch of nblocks callbacks"""
    _fields_ = [("kernel", C.c_int), ("stages", C.c_int), ("cpr", C.c_int), ("ncu", C.c_int), ("device_cus", C.c_int),
                ("chunk_blocks", C.c_int), ("units", C.c_uint), ("runs_per_unit", C.c_uint), ("tiles_per_run", C.c_uint),
                ("runs", C.c_uint), ("wave_slots", C.c_uint), ("workgroups", C.c_uint), ("waves", C.c_uint)]


class SamplesLaunch(C.Structure):
    """acg_lab_samples_launch: the kernel family one launch of a sample format takes, and the streaming kernel's tile geometry"""
    _fields_ = [("family", C.c_int), ("tile_windows", C.c_int), ("stages", C.c_int), ("waves_per_workgroup", C.c_int),
                ("bodies_per_run", C.c_int), ("chunk_blocks", C.c_int), ("runs", C.c_uint), ("waves", C.c_uint)]


assert C.sizeof(ChanStats) == 88
assert C.sizeof(ReasmMsg) == 80 and C.sizeof(ReasmConfig) == 24
assert C.sizeof(Flight) == 120 and C.sizeof(Route) == 56 and C.sizeof(FlightEvent) == 88

BIT_SINK = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_float, C.c_float)

# name -> (restype, argtypes): every symbol include/acarsdec_amd.h (the product API) and include/acarsdec_amd_lab.h (measurement
# and diagnostics: LAB_SYMBOLS below) declare; the library exports exactly these (tests/test_host_logic.py)
SYMBOLS = {
    "acg_device_count": (C.c_int, []),
    "acg_create": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Config)]),
    "acg_destroy": (None, [C.c_void_p]),
    "acg_strerror": (C.c_char_p, [C.c_int]),
    "acg_last_error": (C.c_char_p, [C.c_void_p]),
    "acg_version": (C.c_char_p, []),
    "acg_rtl_choose_fc": (C.c_uint, [C.c_void_p, C.c_uint, C.c_int]),
    "acg_rtl_taps": (C.c_int, [C.c_int, C.c_uint, C.c_int, C.c_void_p]),
    "acg_set_taps": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "acg_set_channel_streams": (C.c_int, [C.c_void_p, C.c_void_p]),
    "acg_reset": (C.c_int, [C.c_void_p]),
    "acg_process_iq_u8_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "acg_process_iq_u8_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "acg_process_dm_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "acg_process_dm_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]),
    "acg_fir_only_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]),
    "acg_sync": (C.c_int, [C.c_void_p]),
    "acg_soapy_taps": (C.c_int, [C.c_float, C.c_int, C.c_int, C.c_void_p]),
    "acg_sdrplay_taps": (C.c_int, [C.c_float, C.c_uint, C.c_void_p]),
    "acg_airspy_choose_fc": (C.c_uint, [C.c_uint, C.c_uint]),
    "acg_airspy_taps": (C.c_int, [C.c_int, C.c_int, C.c_uint, C.c_void_p]),
    "acg_process_samples_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]),
    "acg_feed_samples_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_size_t]),
    "acg_rate_decim": (C.c_int, [C.c_uint]),
    "acg_rate_window_starts": (C.c_int, [C.c_uint, C.c_ulonglong, C.c_int, C.c_void_p]),
    "acg_rate_taps": (C.c_int, [C.c_uint, C.c_double, C.c_int, C.c_void_p]),
    "acg_set_input_rate": (C.c_int, [C.c_void_p, C.c_uint]),
    "acg_process_rate_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.POINTER(C.c_int),
                                       C.POINTER(C.c_size_t)]),
    "acg_feed_rate_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t]),
    "acg_set_channel_filter": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "acg_channel_filter_taps": (C.c_int, [C.c_uint, C.c_double, C.c_int, C.c_double, C.c_double, C.c_void_p]),
    "acg_process_pcm_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]),
    "acg_feed_pcm_host": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "acg_host_alloc": (C.c_void_p, [C.c_size_t]),
    "acg_host_free": (None, [C.c_void_p]),
    "acg_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "acg_host_unregister": (C.c_int, [C.c_void_p]),
    "acg_drain_frames": (C.c_int, [C.c_void_p, C.POINTER(Frame), C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_frames": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Frame), C.c_int, C.POINTER(C.c_int)]),
    "acg_drain_msgs": (C.c_int, [C.c_void_p, C.POINTER(Msg), C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_msgs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Msg), C.c_int, C.POINTER(C.c_int)]),
    "acg_parse_label_filter": (C.c_int, [C.c_char_p, C.POINTER(MsgFilter)]),
    "acg_set_msg_filter": (C.c_int, [C.c_void_p, C.POINTER(MsgFilter)]),
    "acg_drain_msgs_oooi": (C.c_int, [C.c_void_p, C.POINTER(Msg), C.POINTER(Oooi), C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_msgs_oooi": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Msg), C.POINTER(Oooi), C.c_int, C.POINTER(C.c_int)]),
    "acg_flights_enable": (C.c_int, [C.c_void_p, C.POINTER(FlightConfig)]),
    "acg_flight_snapshot": (C.c_int, [C.c_void_p, C.POINTER(Flight), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "acg_drain_routes": (C.c_int, [C.c_void_p, C.POINTER(Route), C.c_int, C.POINTER(C.c_int)]),
    "acg_flights_set_channels": (C.c_int, [C.c_void_p, C.c_void_p]),
    "acg_flights_export": (C.c_int, [C.c_void_p, C.c_int]),
    "acg_drain_flight_events": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_flight_events_check": (C.c_int, [C.c_void_p, C.c_int]),
    "acg_flights_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "acg_flights_commit": (C.c_int, [C.c_void_p]),
    "acg_reasm_enable": (C.c_int, [C.c_void_p, C.POINTER(ReasmConfig)]),
    "acg_drain_msgs_reasm": (C.c_int, [C.c_void_p, C.POINTER(Msg), C.POINTER(Oooi), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_msgs_reasm": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Msg), C.POINTER(Oooi), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_drain_reassembled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                        C.POINTER(C.c_int)]),
    "acg_reasm_status_name": (C.c_char_p, [C.c_int]),
    "acg_flight_text_enable": (C.c_int, [C.c_void_p, C.POINTER(FlightTextConfig)]),
    "acg_flight_monitor_text": (C.c_int, [C.c_void_p, C.c_longlong, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                          C.POINTER(C.c_int)]),
    "acg_drain_routes_json": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "acg_json_enable": (C.c_int, [C.c_void_p, C.POINTER(JsonConfig), C.c_void_p]),
    "acg_drain_json": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "acg_collect_json": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "acg_text_enable": (C.c_int, [C.c_void_p, C.POINTER(TextConfig), C.c_void_p]),
    "acg_drain_text": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_text": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_outputs_config_check": (C.c_int, [C.POINTER(OutputsConfig)]),
    "acg_outputs_enable": (C.c_int, [C.c_void_p, C.POINTER(OutputsConfig), C.c_void_p]),
    "acg_drain_outputs": (C.c_int, [C.c_void_p, C.POINTER(OutBuf), C.c_int, C.POINTER(C.c_int)]),
    "acg_collect_outputs": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(OutBuf), C.c_int, C.POINTER(C.c_int)]),
    "acg_channel_numbers_check": (C.c_int, [C.c_void_p, C.c_int]),
    "acg_set_channel_numbers": (C.c_int, [C.c_void_p, C.c_void_p]),
    "acg_sink_keys": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_stats_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "acg_stats_read": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_ulonglong)]),
    "acg_read_bits": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "acg_read_bits_all": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "acg_bit_capacity": (C.c_int, [C.c_void_p]),
    "acg_max_lag": (C.c_int, [C.c_void_p]),
    "acg_read_dm": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int]),
    "acg_get_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ChanState)]),
    "acg_set_state": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(ChanState)]),
    "acg_get_state_n": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(ChanState)]),
    "acg_set_state_n": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(ChanState)]),
    "acg_get_block_text": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "acg_set_block_text": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "acg_read_dm_n": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_int]),
    "acg_replay_bits": (C.c_int, [C.c_void_p, BIT_SINK, C.c_void_p]),
    "acg_get_timing": (C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                 C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "acg_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
}

# include/acarsdec_amd_lab.h: measurement / diagnostics (exported by the product library too: bench.py times the product)
LAB_SYMBOLS = {
    "acg_placement_trial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_double)]),
    "acg_placement_trial_samples": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_void_p,
                                              C.POINTER(C.c_double)]),
    "acg_tune": (C.c_int, [C.c_char_p, C.c_char_p]),
    "acg_is_lab_build": (C.c_int, []),
    "acg_fill_random_u8_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_size_t, C.c_uint64, C.c_void_p]),
    "acg_synth_iq_u8_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_uint64, C.c_void_p]),
    "acg_probe_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "acg_probe_read_dev": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_double)]),
    "acg_selftest_div2": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "acg_selftest_sincos": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]),
    "acg_selftest_msg_labels": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(MsgFilter), C.c_void_p, C.POINTER(Oooi)]),
    "acg_selftest_flights": (C.c_int, [C.POINTER(Msg), C.POINTER(C.c_int), C.c_int, C.POINTER(FlightConfig), C.POINTER(MsgFilter),
                                       C.POINTER(Flight), C.c_int, C.POINTER(C.c_int), C.POINTER(Route), C.c_int, C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    "acg_selftest_flights_sharded": (C.c_int, [C.POINTER(Msg), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(FlightConfig), C.POINTER(MsgFilter),
                                               C.POINTER(Flight), C.c_int, C.POINTER(C.c_int), C.POINTER(Route), C.c_int, C.POINTER(C.c_int),
                                               C.POINTER(C.c_int), C.POINTER(C.c_float)]),
    "acg_selftest_reasm": (C.c_int, [C.POINTER(Msg), C.POINTER(C.c_int), C.c_int, C.POINTER(ReasmConfig), C.POINTER(MsgFilter), C.c_void_p,
                                     C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p]),
    "acg_selftest_flight_text": (C.c_int, [C.POINTER(Flight), C.c_int, C.POINTER(Route), C.c_int, C.POINTER(FlightConfig),
                                           C.POINTER(FlightTextConfig), C.c_longlong, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t),
                                           C.POINTER(C.c_int), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "acg_selftest_msg_json": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(MsgFilter), C.POINTER(JsonConfig), C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    "acg_lab_json_level_guard": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint)]),
    "acg_selftest_msg_text": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(MsgFilter), C.POINTER(TextConfig), C.c_void_p, C.c_int,
                                        C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_void_p, C.POINTER(C.c_int)]),
    "acg_lab_text_level_guard": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint)]),
    "acg_lab_time_sink_passes": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(JsonConfig), C.POINTER(TextConfig), C.c_int, C.c_int, C.c_int,
                                           C.c_void_p]),
    "acg_selftest_outputs": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(MsgFilter), C.POINTER(OutputsConfig), C.c_void_p, C.c_int,
                                       C.POINTER(OutBuf), C.POINTER(C.c_int)]),
    "acg_lab_outputs_level_guard": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint)]),
    "acg_lab_time_output_passes": (C.c_int, [C.POINTER(Msg), C.c_int, C.POINTER(OutputsConfig), C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "acg_lab_set_block_counter": (C.c_int, [C.c_void_p, C.c_uint]),
    "acg_lab_block_ring_size": (C.c_uint, [C.c_void_p]),
    "acg_lab_set_stream_counters": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_longlong, C.c_longlong]),
    "acg_lab_fir_launch_shape": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(LaunchShape)]),
    "acg_lab_samples_launch_shape": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.POINTER(SamplesLaunch)]),
    "acg_lab_pcm_deinterleave": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_float]),
}
# declared in acarsdec_amd_lab.h, present in the stamp build only (-DACG_MSK_STAMP)
STAMP_SYMBOLS = ("acg_msk_stamp_read", "acg_msk_lanes_per_channel")

_lib = None
_lab = None


def _open(path):
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    try:
        # PyTorch bundles its own libamdhip64.so.7; importing it first makes this library bind
        # to the SAME HIP runtime instance so torch device pointers / streams are usable here.
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is plumbing, not required by the library
        pass
    L = C.CDLL(path)
    for name, (res, args) in list(SYMBOLS.items()) + list(LAB_SYMBOLS.items()):
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    return L


def load(lab=False):
    """Load the native library.  Raises (never falls back) if it is missing.  lab=True: the lab build (a second, independent
    library with its own tuning table), for tests and probes that need a measurement variant."""
    global _lib, _lab
    if lab:
        if _lab is None:
            _lab = _open(LAB_PATH)
            assert _lab.acg_is_lab_build() == 1
        return _lab
    if _lib is None:
        _lib = _open(LIB_PATH)
    return _lib


def tune(name, value, lab=False):
    """Measurement switch NAME (ACG_...) := value for the following launches; None removes the override.  The library
    reads the environment only once, at its first look-up, so changing os.environ later has no effect: use this."""
    rc = load(lab).acg_tune(name.encode(), None if value is None else str(value).encode())
    if rc != OK:
        raise AcgError(rc, "acg_tune(%s)" % name)


class AcgError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        super().__init__("acarsdec_amd error %d: %s %s" % (code, load().acg_strerror(code).decode(), msg))
