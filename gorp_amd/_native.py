"""ctypes binding of libgorp_hip.so (the C ABI in include/gorp_hip.h).

The library is the product: if it is missing this module raises -- there is no
Python or CPU fallback for the hot path.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgorp_hip.so")

GX_OK = 0
GX_E_REGEX_SYNTAX = 1
GX_E_UNSUPPORTED_CONSTRUCT = 2
GX_E_DEVICE = 3
GX_E_ARG = 4
GX_E_NOMEM = 5
GX_E_LIMIT = 6
GX_E_DEFINITION = 7
GX_CREATE_HOST_ONLY = 1
GX_CREATE_TIER_L2 = 2
GX_CREATE_NO_TILES = 4
GX_CREATE_NO_FUSED = 8
GX_CREATE_TIER_RECORDS = 16
GX_CREATE_TIER_RECORDS_GLOBAL = 32
GX_CREATE_TIER_HOP = 64
GX_CREATE_RESIDENT_ONE = 128
GX_CREATE_PROGRAMS = 256
(GX_WHERE_SET, GX_WHERE_EQ, GX_WHERE_PREFIX, GX_WHERE_SUFFIX, GX_WHERE_CONTAINS, GX_WHERE_INT_EQ, GX_WHERE_INT_LT, GX_WHERE_INT_LE, GX_WHERE_INT_GT,
 GX_WHERE_INT_GE) = range(10)
GX_KERNEL_AUTO, GX_KERNEL_TILES, GX_KERNEL_SLICES, GX_KERNEL_PER_LINE, GX_KERNEL_LANES, GX_KERNEL_HOPS, GX_KERNEL_HOP_SLICES = 0, 1, 2, 3, 4, 5, 6

# every symbol include/gorp_hip.h declares
SYMBOLS = [
    "gx_create_from_patterns", "gx_blob_size", "gx_blob_copy", "gx_create_from_blob", "gx_destroy",
    "gx_num_extractions", "gx_num_groups", "gx_max_groups", "gx_stat", "gx_extract_batch",
    "gx_extract_one_utf16", "gx_match_one_utf16", "gx_last_error", "gx_device_count",
    "gx_quote_literal_as_regexp", "gx_massage_regexp_for_automaton", "gx_massage_regexp_for_jdk",
    "gx_create_from_definition", "gx_definition_to_json",
    "gx_extraction_name", "gx_extractor_name", "gx_extraction_append_json",
    "gx_split_lines", "gx_results_to_jsonl", "gx_set_extraction_meta",
    "gx_extraction_append_count", "gx_extraction_append_key", "gx_extraction_append_value_json",
    "gx_pack_results", "gx_unpack_results", "gx_unpack_results8", "gx_text_to_jsonl", "gx_capture_one_utf16",
    "gx_match_batch", "gx_state_accepts", "gx_set_device", "gx_handle_device", "gx_extract_batch_multi",
    "gx_host_register", "gx_host_unregister", "gx_split_lines_max", "gx_extract_batch_multi_device",
    "gx_create_on_devices", "gx_gather_rows", "gx_gather_wait", "gx_release_scratch",
    "gx_count_outcomes", "gx_select_lines", "gx_text_select", "gx_utf8_to_utf16",
    "gx_partition_lines", "gx_text_to_jsonl_by_extraction",
    "gx_select_lines_where", "gx_text_select_where",
    "gx_capture_stats", "gx_text_capture_stats",
    "gx_group_lines", "gx_text_group_lines",
    "gx_top_lines", "gx_text_top_lines",
    "gx_capture_quantiles", "gx_text_capture_quantiles",
    "gx_group_quantiles", "gx_text_group_quantiles",
    "gx_top_groups", "gx_text_top_groups",
    "gx_lines_by_key", "gx_text_lines_by_key",
    "gx_group_pairs", "gx_text_group_pairs",
    "gx_bucket_lines", "gx_text_bucket_lines",
    "gx_group_series", "gx_text_group_series",
    "gx_group_sessions", "gx_text_group_sessions",
    "gx_group_spans", "gx_text_group_spans",
    "gx_group_windows", "gx_text_group_windows",
    "gx_lookup_lines", "gx_text_lookup_lines",
    "gx_sort_lines", "gx_text_sort_lines",
    "gx_set_number_format", "gx_get_number_format", "gx_parse_number",
]


class gx_batch_opts(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("device_pointers", C.c_uint32),
        ("offsets64", C.c_uint32),
        ("match_only", C.c_uint32),
        ("stream", C.c_void_p),
        ("no_sync", C.c_uint32),
        ("line_bytes_hint", C.c_uint32),
        ("strip_eol", C.c_uint32),
        ("utf8_passthrough", C.c_uint32),
        ("utf16", C.c_uint32),
        ("kernel", C.c_uint32),
        ("compact_results", C.c_uint32),
        ("uneven_lines", C.c_uint32),
        ("overflow", C.c_void_p),
        ("max_line_bytes", C.c_uint32),
        ("utf8", C.c_uint32),
        ("utf8_line_flags", C.c_void_p),
    ]


class gx_where_term(C.Structure):
    _fields_ = [("extraction", C.c_int32), ("group", C.c_int32), ("op", C.c_uint32), ("negate", C.c_uint32), ("text", C.c_void_p),
                ("text_units", C.c_uint32), ("number", C.c_int64)]


class gx_measure(C.Structure):
    _fields_ = [("extraction", C.c_int32), ("group", C.c_int32), ("edges", C.c_void_p), ("n_edges", C.c_uint32)]


class gx_measure_stats(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("numbers", C.c_uint64), ("unset", C.c_uint64), ("not_numbers", C.c_uint64), ("min", C.c_int64), ("max", C.c_int64),
                ("sum_lo", C.c_uint64), ("sum_hi", C.c_int64)]


GX_NUMBER_LONG, GX_NUMBER_DECIMAL, GX_NUMBER_ISO8601, GX_NUMBER_CLF = range(4)


class gx_number_format(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("scale", C.c_uint32)]


GX_GROUP_WEAK_HASH = 1
GX_TOP_SMALLEST = 1
GX_TOP_MAX_LINES = 4096
GX_QUANTILE_MAX = 16
GX_RANK_LINES, GX_RANK_NUMBERS, GX_RANK_SUM, GX_RANK_MAX, GX_RANK_MIN = range(5)
GX_TOP_GROUPS_SMALLEST = 2
GX_TOP_GROUPS_MAX = 4096
GX_BY_KEY_ALL_DIGITS = 2
GX_BUCKET_ALL_DIGITS = 2
GX_SPAN_BEGIN, GX_SPAN_END = 1, 2
GX_SORT_DESCENDING, GX_SORT_CARRY, GX_SORT_REST_LAST, GX_SORT_ALL_DIGITS = 1, 2, 4, 8


class gx_group_part(C.Structure):
    _fields_ = [("extraction", C.c_int32), ("key_group", C.c_int32), ("value_group", C.c_int32), ("reserved", C.c_uint32)]


class gx_top_part(C.Structure):
    _fields_ = [("extraction", C.c_int32), ("value_group", C.c_int32)]


class gx_top_totals(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("numbers", C.c_uint64), ("unset", C.c_uint64), ("not_numbers", C.c_uint64), ("n_top", C.c_uint64),
                ("units_top", C.c_uint64), ("last_value", C.c_int64), ("ties_left", C.c_uint64)]


class gx_quantile(C.Structure):
    _fields_ = [("num", C.c_uint32), ("den", C.c_uint32)]


class gx_quantile_out(C.Structure):
    _fields_ = [("value", C.c_int64), ("rank", C.c_uint64), ("below", C.c_uint64), ("equal", C.c_uint64)]


class gx_quantile_totals(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("numbers", C.c_uint64), ("unset", C.c_uint64), ("not_numbers", C.c_uint64)]


class gx_group_out(C.Structure):
    _fields_ = [("key_units", C.c_void_p), ("key_units_cap", C.c_uint64), ("key_offsets", C.c_void_p), ("key_first_line", C.c_void_p),
                ("key_lines", C.c_void_p), ("key_stats", C.c_void_p), ("line_key", C.c_void_p), ("max_keys", C.c_uint64)]


class gx_group_totals(C.Structure):
    _fields_ = [("n_keys", C.c_uint64), ("key_units", C.c_uint64), ("lines", C.c_uint64), ("keyed", C.c_uint64), ("unset", C.c_uint64),
                ("exact", C.c_uint64)]


class gx_top_groups_out(C.Structure):
    _fields_ = [("key_units", C.c_void_p), ("key_units_cap", C.c_uint64), ("key_offsets", C.c_void_p), ("key_number", C.c_void_p),
                ("key_first_line", C.c_void_p), ("key_lines", C.c_void_p), ("key_stats", C.c_void_p), ("line_rank", C.c_void_p), ("cap_keys", C.c_uint64)]


class gx_top_groups_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("candidates", C.c_uint64), ("n_top", C.c_uint64), ("units_top", C.c_uint64), ("last_lo", C.c_uint64),
                ("last_hi", C.c_int64), ("ties_left", C.c_uint64)]


class gx_by_key_out(C.Structure):
    _fields_ = [("out_index", C.c_void_p), ("out_bytes", C.c_void_p), ("out_offsets", C.c_void_p), ("out_ids", C.c_void_p), ("out_caps", C.c_void_p),
                ("cap_lines", C.c_uint64), ("out_bytes_cap", C.c_uint64), ("key_out_lines", C.c_void_p), ("key_out_units", C.c_void_p)]


class gx_by_key_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("keys_kept", C.c_uint64), ("lines_out", C.c_uint64), ("units_out", C.c_uint64)]


class gx_sort_out(C.Structure):
    _fields_ = [("out_index", C.c_void_p), ("out_values", C.c_void_p), ("out_class", C.c_void_p), ("out_bytes", C.c_void_p), ("out_offsets", C.c_void_p),
                ("out_ids", C.c_void_p), ("out_caps", C.c_void_p), ("cap_lines", C.c_uint64), ("out_bytes_cap", C.c_uint64)]


class gx_sort_totals(C.Structure):
    _fields_ = [("lines", C.c_uint64), ("numbers", C.c_uint64), ("unset", C.c_uint64), ("not_numbers", C.c_uint64), ("carried", C.c_uint64), ("rest", C.c_uint64),
                ("lines_out", C.c_uint64), ("units_out", C.c_uint64), ("first_value", C.c_int64), ("last_value", C.c_int64), ("n_passes", C.c_uint32),
                ("already_ordered", C.c_uint32)]


class gx_sessions_out(C.Structure):
    _fields_ = [("session_key", C.c_void_p), ("session_begin", C.c_void_p), ("session_end", C.c_void_p), ("session_first_line", C.c_void_p),
                ("session_lines", C.c_void_p), ("session_stats", C.c_void_p), ("session_entry_begin", C.c_void_p), ("key_session_begin", C.c_void_p),
                ("entry_line", C.c_void_p), ("line_session", C.c_void_p), ("max_sessions", C.c_uint64), ("max_entries", C.c_uint64)]


class gx_spans_out(C.Structure):
    _fields_ = [("span_key", C.c_void_p), ("span_begin_line", C.c_void_p), ("span_end_line", C.c_void_p), ("span_begin", C.c_void_p), ("span_end", C.c_void_p),
                ("span_duration", C.c_void_p), ("span_class", C.c_void_p), ("key_span_begin", C.c_void_p), ("key_span_stats", C.c_void_p),
                ("key_open_line", C.c_void_p), ("line_span", C.c_void_p), ("line_state", C.c_void_p), ("max_spans", C.c_uint64)]


class gx_windows_out(C.Structure):
    _fields_ = [("entry_line", C.c_void_p), ("entry_key", C.c_void_p), ("entry_time", C.c_void_p), ("entry_window_lines", C.c_void_p),
                ("entry_window_sum", C.c_void_p), ("key_entry_begin", C.c_void_p), ("key_peak_lines", C.c_void_p), ("key_peak_line", C.c_void_p),
                ("line_window_lines", C.c_void_p), ("trip_key", C.c_void_p), ("trip_line", C.c_void_p), ("trip_time", C.c_void_p), ("trip_entry", C.c_void_p),
                ("key_trip_begin", C.c_void_p), ("max_entries", C.c_uint64), ("max_trips", C.c_uint64)]


class gx_sessions_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("n_sessions", C.c_uint64), ("entries", C.c_uint64), ("number_unset", C.c_uint64), ("not_numbers", C.c_uint64),
                ("longest_lines", C.c_uint64), ("longest_duration", C.c_uint64), ("first_time", C.c_int64), ("last_time", C.c_int64)]


class gx_windows_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("entries", C.c_uint64), ("number_unset", C.c_uint64), ("not_numbers", C.c_uint64), ("n_trips", C.c_uint64),
                ("tripped_keys", C.c_uint64), ("peak_lines", C.c_uint64), ("peak_line", C.c_uint32), ("peak_key", C.c_uint32), ("first_time", C.c_int64),
                ("last_time", C.c_int64)]


GX_LOOKUP_NONE, GX_LOOKUP_MISS = 0xFFFFFFFF, 0xFFFFFFFE
GX_LOOKUP_KEEP_NOTHING, GX_LOOKUP_KEEP_HITS, GX_LOOKUP_KEEP_OTHERS = range(3)


class gx_lookup_out(C.Structure):
    _fields_ = [("line_entry", C.c_void_p), ("entry_same", C.c_void_p), ("entry_lines", C.c_void_p), ("entry_first_line", C.c_void_p),
                ("entry_stats", C.c_void_p), ("out_index", C.c_void_p), ("out_bytes", C.c_void_p), ("out_offsets", C.c_void_p), ("out_ids", C.c_void_p),
                ("out_caps", C.c_void_p), ("cap_lines", C.c_uint64), ("out_bytes_cap", C.c_uint64)]


class gx_lookup_totals(C.Structure):
    _fields_ = [("entries", C.c_uint64), ("distinct_entries", C.c_uint64), ("hit_entries", C.c_uint64), ("lines", C.c_uint64), ("keyed", C.c_uint64),
                ("unset", C.c_uint64), ("hits", C.c_uint64), ("misses", C.c_uint64), ("lines_out", C.c_uint64), ("units_out", C.c_uint64)]


class gx_spans_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("n_spans", C.c_uint64), ("begins", C.c_uint64), ("ends", C.c_uint64), ("superseded", C.c_uint64),
                ("left_open", C.c_uint64), ("orphan_ends", C.c_uint64), ("out_of_range", C.c_uint64), ("durations", gx_measure_stats)]


class gx_series_out(C.Structure):
    _fields_ = [("bucket_number", C.c_void_p), ("cell_key", C.c_void_p), ("cell_bucket", C.c_void_p), ("cell_first_line", C.c_void_p), ("cell_lines", C.c_void_p),
                ("cell_stats", C.c_void_p), ("key_cell_begin", C.c_void_p), ("line_cell", C.c_void_p), ("max_cells", C.c_uint64), ("max_buckets", C.c_uint64)]


class gx_series_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("n_cells", C.c_uint64), ("n_buckets", C.c_uint64), ("celled", C.c_uint64), ("number_unset", C.c_uint64),
                ("not_numbers", C.c_uint64), ("out_of_range", C.c_uint64), ("cells_exact", C.c_uint64), ("first_bucket", C.c_int64), ("last_bucket", C.c_int64)]


class gx_pairs_out(C.Structure):
    _fields_ = [("pair_units", C.c_void_p), ("pair_units_cap", C.c_uint64), ("pair_offsets", C.c_void_p), ("pair_key", C.c_void_p),
                ("pair_first_line", C.c_void_p), ("pair_lines", C.c_void_p), ("key_pairs", C.c_void_p), ("line_pair", C.c_void_p), ("max_pairs", C.c_uint64)]


class gx_pairs_totals(C.Structure):
    _fields_ = [("group", gx_group_totals), ("n_pairs", C.c_uint64), ("pair_units", C.c_uint64), ("paired", C.c_uint64), ("unpaired", C.c_uint64),
                ("pairs_exact", C.c_uint64)]


class gx_bucket_part(C.Structure):
    _fields_ = [("extraction", C.c_int32), ("number_group", C.c_int32), ("value_group", C.c_int32), ("reserved", C.c_uint32)]


class gx_bucket_out(C.Structure):
    _fields_ = [("bucket_number", C.c_void_p), ("bucket_first_line", C.c_void_p), ("bucket_lines", C.c_void_p), ("bucket_stats", C.c_void_p),
                ("line_bucket", C.c_void_p), ("max_buckets", C.c_uint64)]


class gx_bucket_totals(C.Structure):
    _fields_ = [("n_buckets", C.c_uint64), ("lines", C.c_uint64), ("bucketed", C.c_uint64), ("unset", C.c_uint64), ("not_numbers", C.c_uint64),
                ("out_of_range", C.c_uint64), ("exact", C.c_uint64), ("first_bucket", C.c_int64), ("last_bucket", C.c_int64)]


class gx_device_shard(C.Structure):
    _fields_ = [("handle", C.c_void_p), ("bytes", C.c_void_p), ("offsets", C.c_void_p), ("n", C.c_uint64), ("match_id", C.c_void_p),
                ("caps", C.c_void_p), ("overflow", C.c_void_p), ("stream", C.c_void_p)]


class gx_rows_shard(C.Structure):
    _fields_ = [("handle", C.c_void_p), ("rows", C.c_void_p), ("n", C.c_uint64), ("stream", C.c_void_p)]


_lib = None
_hip_runtime = None


def _load_hip_runtime():
    """libgorp_hip.so is linked without a NEEDED libamdhip64 (see build.py): load the one
    HIP runtime this process will use, globally, before it.  If PyTorch is installed its
    bundled runtime is the one torch will insist on, so take that; otherwise ROCm's."""
    global _hip_runtime
    if _hip_runtime is not None:
        return _hip_runtime
    import importlib.util
    candidates = []
    env = os.environ.get("GORP_HIP_RUNTIME")
    if env:
        candidates.append(env)
    try:
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            candidates.append(os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so"))
    except (ImportError, ValueError):
        pass
    candidates += ["/opt/rocm/lib/libamdhip64.so", "libamdhip64.so"]
    errors = []
    for path in candidates:
        if os.path.isabs(path) and not os.path.exists(path):
            continue
        try:
            _hip_runtime = C.CDLL(path, mode=C.RTLD_GLOBAL)
            return _hip_runtime
        except OSError as e:
            errors.append("%s: %s" % (path, e))
    raise ImportError("gorp_amd: no HIP runtime (libamdhip64) could be loaded: " + "; ".join(errors))


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "gorp_amd: %s not found. Build it with `python -m gorp_amd.build` (hipcc, gfx950). "
            "There is no CPU fallback for the extract path." % LIB_PATH)
    _load_hip_runtime()
    L = C.CDLL(LIB_PATH)
    L.gx_create_from_patterns.argtypes = [C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.c_int32, C.c_uint32,
                                          C.POINTER(C.c_void_p)]
    L.gx_create_from_patterns.restype = C.c_int
    L.gx_blob_size.argtypes = [C.c_void_p]
    L.gx_blob_size.restype = C.c_size_t
    L.gx_blob_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.gx_blob_copy.restype = C.c_int
    L.gx_create_from_blob.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.POINTER(C.c_void_p)]
    L.gx_create_from_blob.restype = C.c_int
    L.gx_destroy.argtypes = [C.c_void_p]
    L.gx_destroy.restype = None
    L.gx_num_extractions.argtypes = [C.c_void_p]
    L.gx_num_extractions.restype = C.c_int32
    L.gx_num_groups.argtypes = [C.c_void_p, C.c_int32]
    L.gx_num_groups.restype = C.c_int32
    L.gx_max_groups.argtypes = [C.c_void_p]
    L.gx_max_groups.restype = C.c_int32
    L.gx_stat.argtypes = [C.c_void_p, C.c_int32]
    L.gx_stat.restype = C.c_int64
    L.gx_extract_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.POINTER(gx_batch_opts)]
    L.gx_extract_batch.restype = C.c_int
    L.gx_extract_one_utf16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    L.gx_extract_one_utf16.restype = C.c_int
    L.gx_match_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_match_batch.restype = C.c_int
    L.gx_state_accepts.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    L.gx_state_accepts.restype = C.c_int
    L.gx_capture_one_utf16.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_void_p]
    L.gx_capture_one_utf16.restype = C.c_int
    L.gx_match_one_utf16.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
    L.gx_match_one_utf16.restype = C.c_int
    L.gx_last_error.argtypes = []
    L.gx_last_error.restype = C.c_char_p
    L.gx_device_count.argtypes = []
    L.gx_device_count.restype = C.c_int
    L.gx_set_device.argtypes = [C.c_int]
    L.gx_set_device.restype = C.c_int
    L.gx_handle_device.argtypes = [C.c_void_p]
    L.gx_handle_device.restype = C.c_int
    L.gx_extract_batch_multi.argtypes = [C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                         C.POINTER(gx_batch_opts)]
    L.gx_extract_batch_multi.restype = C.c_int
    L.gx_extract_batch_multi_device.argtypes = [C.POINTER(gx_device_shard), C.c_int32, C.POINTER(gx_batch_opts)]
    L.gx_extract_batch_multi_device.restype = C.c_int
    L.gx_create_on_devices.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_int32), C.c_int32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.gx_create_on_devices.restype = C.c_int
    L.gx_gather_rows.argtypes = [C.POINTER(gx_rows_shard), C.c_int32, C.c_uint32, C.c_int32, C.c_void_p, C.c_int32]
    L.gx_gather_rows.restype = C.c_int
    L.gx_gather_wait.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
    L.gx_gather_wait.restype = C.c_int
    L.gx_release_scratch.argtypes = [C.c_int]
    L.gx_release_scratch.restype = C.c_int
    L.gx_host_register.argtypes = [C.c_void_p, C.c_size_t]
    L.gx_host_register.restype = C.c_int
    L.gx_host_unregister.argtypes = [C.c_void_p]
    L.gx_host_unregister.restype = C.c_int
    for f in ("gx_quote_literal_as_regexp", "gx_massage_regexp_for_automaton", "gx_massage_regexp_for_jdk"):
        getattr(L, f).argtypes = [C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        getattr(L, f).restype = C.c_int
    L.gx_create_from_definition.argtypes = [C.c_char_p, C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
    L.gx_create_from_definition.restype = C.c_int
    L.gx_definition_to_json.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.gx_definition_to_json.restype = C.c_int
    L.gx_extraction_name.argtypes = [C.c_void_p, C.c_int32]
    L.gx_extraction_name.restype = C.c_char_p
    L.gx_extractor_name.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
    L.gx_extractor_name.restype = C.c_char_p
    L.gx_extraction_append_json.argtypes = [C.c_void_p, C.c_int32]
    L.gx_extraction_append_json.restype = C.c_char_p
    L.gx_split_lines.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                 C.POINTER(gx_batch_opts)]
    L.gx_split_lines.restype = C.c_int
    L.gx_split_lines_max.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                     C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_split_lines_max.restype = C.c_int
    L.gx_results_to_jsonl.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_char_p,
                                      C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_results_to_jsonl.restype = C.c_int
    L.gx_set_extraction_meta.argtypes = [C.c_void_p, C.c_int32, C.c_char_p, C.POINTER(C.c_char_p), C.c_int32, C.c_char_p]
    L.gx_set_extraction_meta.restype = C.c_int
    L.gx_set_number_format.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(gx_number_format)]
    L.gx_set_number_format.restype = C.c_int
    L.gx_get_number_format.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(gx_number_format)]
    L.gx_get_number_format.restype = C.c_int
    L.gx_parse_number.argtypes = [C.POINTER(gx_number_format), C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.gx_parse_number.restype = C.c_int
    L.gx_text_to_jsonl.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_to_jsonl.restype = C.c_int
    L.gx_count_outcomes.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_count_outcomes.restype = C.c_int
    L.gx_select_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                  C.POINTER(gx_batch_opts)]
    L.gx_select_lines.restype = C.c_int
    L.gx_text_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                 C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_select.restype = C.c_int
    L.gx_select_lines_where.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(gx_where_term),
                                        C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_select_lines_where.restype = C.c_int
    L.gx_text_select_where.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(gx_where_term), C.c_uint32, C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_select_where.restype = C.c_int
    L.gx_capture_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_measure), C.c_uint32,
                                   C.POINTER(gx_where_term), C.c_uint32, C.POINTER(gx_measure_stats), C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_capture_stats.restype = C.c_int
    L.gx_text_capture_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_measure), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                        C.POINTER(gx_measure_stats), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_capture_stats.restype = C.c_int
    L.gx_group_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32,
                                 C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_group_totals),
                                 C.POINTER(gx_batch_opts)]
    L.gx_group_lines.restype = C.c_int
    L.gx_text_group_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                      C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_group_totals), C.c_void_p, C.POINTER(C.c_uint64),
                                      C.POINTER(gx_batch_opts)]
    L.gx_text_group_lines.restype = C.c_int
    L.gx_top_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_top_part), C.c_uint32,
                               C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                               C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(gx_top_totals), C.POINTER(gx_batch_opts)]
    L.gx_top_lines.restype = C.c_int
    L.gx_text_top_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_top_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                    C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(gx_top_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_top_lines.restype = C.c_int
    L.gx_capture_quantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_top_part), C.c_uint32,
                                       C.POINTER(gx_where_term), C.c_uint32, C.POINTER(gx_quantile), C.c_uint32, C.POINTER(gx_quantile_out),
                                       C.POINTER(gx_quantile_totals), C.POINTER(gx_batch_opts)]
    L.gx_capture_quantiles.restype = C.c_int
    L.gx_text_capture_quantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_top_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                            C.POINTER(gx_quantile), C.c_uint32, C.POINTER(gx_quantile_out), C.POINTER(gx_quantile_totals), C.c_void_p,
                                            C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_capture_quantiles.restype = C.c_int
    L.gx_group_quantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32,
                                     C.POINTER(gx_where_term), C.c_uint32, C.POINTER(gx_quantile), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out),
                                     C.c_void_p, C.POINTER(gx_group_totals), C.POINTER(gx_batch_opts)]
    L.gx_group_quantiles.restype = C.c_int
    L.gx_text_group_quantiles.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                          C.POINTER(gx_quantile), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.c_void_p,
                                          C.POINTER(gx_group_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_quantiles.restype = C.c_int
    L.gx_top_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32,
                                C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(gx_top_groups_out),
                                C.POINTER(gx_top_groups_totals), C.POINTER(gx_batch_opts)]
    L.gx_top_groups.restype = C.c_int
    L.gx_text_top_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                     C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.POINTER(gx_top_groups_out), C.POINTER(gx_top_groups_totals),
                                     C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_top_groups.restype = C.c_int
    L.gx_lines_by_key.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32,
                                  C.POINTER(gx_where_term), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_by_key_out),
                                  C.POINTER(gx_by_key_totals), C.POINTER(gx_batch_opts)]
    L.gx_lines_by_key.restype = C.c_int
    L.gx_text_lines_by_key.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                       C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(gx_group_out), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.POINTER(gx_by_key_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_lines_by_key.restype = C.c_int
    L.gx_group_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32),
                                 C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_pairs_out), C.POINTER(gx_pairs_totals),
                                 C.POINTER(gx_batch_opts)]
    L.gx_group_pairs.restype = C.c_int
    L.gx_text_group_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(gx_where_term),
                                      C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_pairs_out), C.POINTER(gx_pairs_totals), C.c_void_p,
                                      C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_pairs.restype = C.c_int
    L.gx_group_series.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32),
                                  C.c_int64, C.c_int64, C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_series_out),
                                  C.POINTER(gx_series_totals), C.POINTER(gx_batch_opts)]
    L.gx_group_series.restype = C.c_int
    L.gx_text_group_series.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32), C.c_int64, C.c_int64,
                                       C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_series_out),
                                       C.POINTER(gx_series_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_series.restype = C.c_int
    L.gx_group_sessions.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32),
                                    C.c_int64, C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_sessions_out),
                                    C.POINTER(gx_sessions_totals), C.POINTER(gx_batch_opts)]
    L.gx_group_sessions.restype = C.c_int
    L.gx_text_group_sessions.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32), C.c_int64,
                                         C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_sessions_out),
                                         C.POINTER(gx_sessions_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_sessions.restype = C.c_int
    L.gx_group_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32),
                                   C.c_int64, C.c_uint32, C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_windows_out),
                                   C.POINTER(gx_windows_totals), C.POINTER(gx_batch_opts)]
    L.gx_group_windows.restype = C.c_int
    L.gx_text_group_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32), C.c_int64, C.c_uint32,
                                        C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_windows_out),
                                        C.POINTER(gx_windows_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_windows.restype = C.c_int
    L.gx_lookup_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32,
                                  C.POINTER(gx_where_term), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(gx_lookup_out),
                                  C.POINTER(gx_lookup_totals), C.POINTER(gx_batch_opts)]
    L.gx_lookup_lines.restype = C.c_int
    L.gx_text_lookup_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(gx_lookup_out), C.c_void_p, C.c_uint64,
                                       C.c_void_p, C.c_void_p, C.POINTER(gx_lookup_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_lookup_lines.restype = C.c_int
    L.gx_group_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32),
                                 C.POINTER(C.c_uint32), C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_spans_out),
                                 C.POINTER(gx_spans_totals), C.POINTER(gx_batch_opts)]
    L.gx_group_spans.restype = C.c_int
    L.gx_text_group_spans.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_group_part), C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_uint32),
                                      C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_group_out), C.POINTER(gx_spans_out),
                                      C.POINTER(gx_spans_totals), C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_group_spans.restype = C.c_int
    L.gx_bucket_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_bucket_part), C.c_uint32, C.c_int64, C.c_int64,
                                  C.POINTER(gx_where_term), C.c_uint32, C.c_uint32, C.POINTER(gx_bucket_out), C.POINTER(gx_bucket_totals), C.POINTER(gx_batch_opts)]
    L.gx_bucket_lines.restype = C.c_int
    L.gx_text_bucket_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_bucket_part), C.c_uint32, C.c_int64, C.c_int64, C.POINTER(gx_where_term),
                                       C.c_uint32, C.c_uint32, C.POINTER(gx_bucket_out), C.POINTER(gx_bucket_totals), C.c_void_p, C.POINTER(C.c_uint64),
                                       C.POINTER(gx_batch_opts)]
    L.gx_text_bucket_lines.restype = C.c_int
    L.gx_sort_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(gx_top_part), C.c_uint32, C.POINTER(gx_where_term),
                                C.c_uint32, C.c_uint32, C.POINTER(gx_sort_out), C.POINTER(gx_sort_totals), C.POINTER(gx_batch_opts)]
    L.gx_sort_lines.restype = C.c_int
    L.gx_text_sort_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(gx_top_part), C.c_uint32, C.POINTER(gx_where_term), C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(gx_sort_totals), C.c_void_p,
                                     C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_sort_lines.restype = C.c_int
    L.gx_partition_lines.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_partition_lines.restype = C.c_int
    L.gx_text_to_jsonl_by_extraction.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                                 C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_text_to_jsonl_by_extraction.restype = C.c_int
    L.gx_utf8_to_utf16.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64),
                                   C.POINTER(gx_batch_opts)]
    L.gx_utf8_to_utf16.restype = C.c_int
    L.gx_pack_results.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(gx_batch_opts)]
    L.gx_pack_results.restype = C.c_int
    L.gx_unpack_results.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_unpack_results.restype = C.c_int
    L.gx_unpack_results8.argtypes = [C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(gx_batch_opts)]
    L.gx_unpack_results8.restype = C.c_int
    L.gx_extraction_append_count.argtypes = [C.c_void_p, C.c_int32]
    L.gx_extraction_append_count.restype = C.c_int32
    for f in ("gx_extraction_append_key", "gx_extraction_append_value_json"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        getattr(L, f).restype = C.c_char_p
    _lib = L
    return L


def last_error():
    m = lib().gx_last_error()
    return m.decode("utf-8", "replace") if m else ""
