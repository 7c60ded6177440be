"""Host-side mirror of the reference's API for the match-and-extract path,
bound to libgorp_hip.so through its C ABI (include/gorp_hip.h).

Names and behaviour follow salesforce/gorp (core/ = gorp-core/src/main/java/com/salesforce/gorp/):
    Gorp.construct / extract / extractSafe     core/Gorp.java:50-92,145-186
    PolyMatcher.create / match                 core/autom/PolyMatcher.java:64-70,123-133
    ExtractionResult.getId / asMap             core/ExtractionResult.java:39-88
    ExtractionException                        core/ExtractionException.java:15-34
    RegexHelper.*                              core/util/RegexHelper.java
plus what the reference lacks and the GPU needs: extract_batch over a CSR
byte buffer.  All matching runs in the HIP kernels; nothing here computes a
match on the CPU.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from . import _native as N


class GorpError(Exception):
    """A C-ABI call failed (code = GX_E_*)."""

    def __init__(self, code, message):
        super().__init__("%s (gx error %d)" % (message, code))
        self.code = code
        self.message = message


class DefinitionParseException(GorpError):
    """core/DefinitionParseException.java -- definition could not be turned into tables."""


class ExtractionException(Exception):
    """core/ExtractionException.java:15-34 -- the multi-matcher chose an extraction whose
    generated regexp then failed to match (core/Gorp.java:173-177)."""

    def __init__(self, input_line, message):
        super().__init__(message)
        self.input = input_line

    def getInput(self):
        return self.input


def _check(rc):
    if rc != N.GX_OK:
        raise GorpError(rc, N.last_error())


# ---------------------------------------------------------------------------
# RegexHelper (core/util/RegexHelper.java) -- implemented in gx_host.cpp
# ---------------------------------------------------------------------------
def _c_text(text):
    """A definition's text as the C ABI takes it: a C string, which would end at a U+0000 silently -- refused instead (the reference's
    Strings may hold one)."""
    if "\x00" in text:
        raise DefinitionParseException(N.GX_E_UNSUPPORTED_CONSTRUCT, "a definition cannot hold U+0000: the library takes C strings "
                                       "(the class [^\\u0001-\\uffff], its bounds written as characters, matches one)")
    return text.encode("utf-8")


def _string_call(fn, text):
    raw = _c_text(text)
    cap = 8 * len(raw) + 64
    buf = C.create_string_buffer(cap)
    n = C.c_size_t(0)
    rc = fn(raw, buf, cap, C.byref(n))
    if rc == N.GX_E_ARG and n.value + 1 > cap:
        cap = n.value + 1
        buf = C.create_string_buffer(cap)
        rc = fn(raw, buf, cap, C.byref(n))
    if rc == N.GX_E_REGEX_SYNTAX:
        raise ValueError(N.last_error())  # IllegalArgumentException in the reference
    _check(rc)
    return buf.raw[:n.value].decode("utf-8")


class RegexHelper:
    @staticmethod
    def quoteLiteralAsRegexp(text):
        return _string_call(N.lib().gx_quote_literal_as_regexp, text)

    @staticmethod
    def massageRegexpForAutomaton(pattern):
        return _string_call(N.lib().gx_massage_regexp_for_automaton, pattern)

    @staticmethod
    def massageRegexpForJDK(pattern):
        return _string_call(N.lib().gx_massage_regexp_for_jdk, pattern)


# ---------------------------------------------------------------------------
# Flattened extraction -> the two regex strings (Gorp._buildExtractor, core/Gorp.java:94-129)
# ---------------------------------------------------------------------------
class FlattenedExtraction:
    """core/model/FlattenedExtraction.java:18-36: a named, ordered piece list.

    pieces: ["text", s] (LiteralText) | ["pattern", s] (LiteralPattern)
            | ["extractor", name, [pieces]] (ExtractorExpression)
    """

    def __init__(self, name, pieces, append=None):
        self.name = name
        self.pieces = pieces
        self.append = append

    def getExtractorNames(self):
        """Extractor names in pre-order == capture group order (core/model/CookedDefinitions.java:444-451)."""
        names = []

        def walk(p):
            if p[0] == "extractor":
                names.append(p[1])
                for c in p[2]:
                    walk(c)

        for p in self.pieces:
            walk(p)
        return names

    def build(self, cooker=None):
        """Gorp._buildExtractor (core/Gorp.java:94-129) over all pieces: the automaton regexp is always built the
        reference's way; the capture-side regexp goes through the ExtractionCooker's append* methods.
        Returns (automaton regexp, cooker regexp, extractor names)."""
        cooker = cooker or HipExtractionCooker.instance()
        autom, regexp = [], []

        def walk(p):
            kind = p[0]
            if kind == "pattern":                       # LiteralPattern, Gorp.java:98-108
                autom.append(RegexHelper.massageRegexpForAutomaton(p[1]))
                cooker.appendPattern(p[1], regexp)
            elif kind == "text":                        # LiteralText, :109-114
                autom.append(RegexHelper.quoteLiteralAsRegexp(p[1]))
                cooker.appendLiteral(p[1], regexp)
            elif kind == "extractor":                   # ExtractorExpression, :115-127
                autom.append("(")
                cooker.appendStartExpression(regexp)
                for c in p[2]:
                    walk(c)
                autom.append(")")
                cooker.appendFinishExpression(regexp)
            else:
                raise DefinitionParseException(N.GX_E_ARG, "Unrecognized DefPiece in FlattenedExtraction: %r" % (kind,))

        for p in self.pieces:
            walk(p)
        return "".join(autom), "".join(regexp), self.getExtractorNames()


class CookedExtraction:
    """core/model/CookedExtraction.java:18-66 (data only; matching happens on the GPU)."""

    def __init__(self, index, name, regexp_source, extractor_names, append=None):
        self._index = index
        self._name = name
        self._regexpSource = regexp_source
        self._extractorNames = list(extractor_names)
        self._append = append
        self._gorp_handle = None  # set by Gorp: match() runs on the definition's device tables

    def getName(self):
        return self._name

    def getExtra(self):
        return self._append

    def getRegexpSource(self):
        return self._regexpSource

    def getRegexpDesc(self):
        return self._regexpSource

    def match(self, input):
        """CookedExtraction.match(String) (core/model/CookedExtraction.java:61): this extraction's capture regexp
        alone -- ExtractionResult or None.  Runs on the GPU (gx_capture_one_utf16); needs the handle that
        Gorp.construct attached."""
        if self._gorp_handle is None:
            raise GorpError(N.GX_E_ARG, "CookedExtraction.match: not attached to a Gorp (use Gorp.construct)")
        a = _utf16(input)
        matched = C.c_int32(0)
        caps = np.full(2 * max(1, N.lib().gx_max_groups(self._gorp_handle.ptr)), -1, np.int32)
        _check(N.lib().gx_capture_one_utf16(self._gorp_handle.ptr, self._index, a.ctypes.data if len(a) else None, len(a),
                                            C.byref(matched), caps.ctypes.data))
        if not matched.value:
            return None
        values = []
        for g in range(len(self._extractorNames)):
            b, e = int(caps[2 * g]), int(caps[2 * g + 1])
            values.append(None if b < 0 else a[b:e].tobytes().decode("utf-16-le", "surrogatepass"))
        return ExtractionResult(self._name, input, self, self._extractorNames, values)


class ExtractionCooker:
    """core/ExtractionCooker.java:16-30 -- the reference's plugin API for the capture backend: a factory that turns a
    FlattenedExtraction into a CookedExtraction and says how pieces are spelled in the backend's regexp dialect.
    `buffer` is a list of string fragments (the StringBuilder)."""

    def cook(self, index, regexpSource, extr):
        raise NotImplementedError

    def appendPattern(self, pattern, buffer):
        raise NotImplementedError

    def appendLiteral(self, literal, buffer):
        raise NotImplementedError

    def appendStartExpression(self, buffer):
        raise NotImplementedError

    def appendFinishExpression(self, buffer):
        raise NotImplementedError


class HipExtractionCooker(ExtractionCooker):
    """The backend of this package, plugged in where the reference plugs JDKRegexpExtractionCooker
    (core/jdkre/JDKRegexpExtractionCooker.java:20-42): same dialect (java.util.regex), so the append* methods are the
    same string rewrites; cook() keeps the data of the CookedExtraction -- the capture regexps of all extractions are
    compiled together, with the match automaton, into the device tables by Gorp.construct (gx_create_from_patterns),
    because one line at a time through CookedExtraction.match would leave the GPU idle."""

    _INSTANCE = None

    @classmethod
    def instance(cls):
        if cls._INSTANCE is None:
            cls._INSTANCE = cls()
        return cls._INSTANCE

    def cook(self, index, regexpSource, extr):
        return CookedExtraction(index, extr.name, regexpSource, extr.getExtractorNames(), extr.append)

    def appendPattern(self, pattern, buffer):
        buffer.append(RegexHelper.massageRegexpForJDK(pattern))

    def appendLiteral(self, literal, buffer):
        buffer.append(RegexHelper.quoteLiteralAsRegexp(literal))

    def appendStartExpression(self, buffer):
        buffer.append("(")

    def appendFinishExpression(self, buffer):
        buffer.append(")")


class ExtractionResult:
    """core/ExtractionResult.java:18-89."""

    def __init__(self, id_, input_line, extraction, names, values):
        self._id = id_
        self._input = input_line
        self._matchedExtraction = extraction
        self._extractorNames = names
        self._extractedValues = values

    def getId(self):
        return self._id

    def getInput(self):
        return self._input

    def getMatchedExtraction(self):
        return self._matchedExtraction

    def getExtra(self):
        return self._matchedExtraction.getExtra()

    def asMap(self, idAs=None):
        result = {}
        if idAs is not None:
            result[idAs] = self._id
        for n, v in zip(self._extractorNames, self._extractedValues):
            result[n] = v
        extra = self.getExtra()
        if extra:
            result.update(extra)
        return result


class WhereTerms:
    """Gorp.where_terms' result: the gx_where_term array of a call, and the literals its text pointers point into."""

    def __init__(self, array, n, literals, units):
        self.array, self.n, self.literals, self.units = array, n, literals, units


class Measures:
    """Gorp.measures' result: the gx_measure array of a call, and the edge arrays its pointers point into."""

    def __init__(self, array, n, edges):
        self.array, self.n, self.edges = array, n, edges

    @property
    def n_bins(self):
        return sum(len(e) + 1 for e in self.edges)


class GroupParts:
    """Gorp.group_parts' result: the gx_group_part array of a call."""

    def __init__(self, array, n):
        self.array, self.n = array, n

    @property
    def has_values(self):
        return any(self.array[t].value_group >= 0 for t in range(self.n))


class BucketParts:
    """Gorp.bucket_parts' result: the gx_bucket_part array of a call."""

    def __init__(self, array, n):
        self.array, self.n = array, n

    @property
    def has_values(self):
        return any(self.array[t].value_group >= 0 for t in range(self.n))


class TopParts:
    """Parts for top_lines (Gorp.top_parts)."""

    def __init__(self, array, n):
        self.array, self.n = array, n


def _utf16(s):
    raw = s.encode("utf-16-le", "surrogatepass")
    return np.frombuffer(raw, dtype=np.uint16).copy() if raw else np.zeros(0, np.uint16)


class _Handle:
    """Owns a gx_handle*."""

    def __init__(self, ptr):
        self.ptr = ptr

    def __del__(self):
        try:
            if self.ptr:
                N.lib().gx_destroy(self.ptr)
                self.ptr = None
        except Exception:
            pass


# Kernel-choice defaults of this module (GX_CREATE_* bits OR-ed into every handle creation, GX_KERNEL_* for batches
# that name none): the tests set them to run whole scenarios on one kernel.  Results never depend on them.
DEFAULT_CREATE_FLAGS = 0
DEFAULT_KERNEL = 0


def _create(autom, jdk, flags):
    L = N.lib()
    flags |= DEFAULT_CREATE_FLAGS
    n = len(autom)
    A = (C.c_char_p * n)(*[_c_text(s) for s in autom])
    J = None
    if jdk is not None:
        J = (C.c_char_p * n)(*[_c_text(s) for s in jdk])
    h = C.c_void_p()
    rc = L.gx_create_from_patterns(A, J, n, flags, C.byref(h))
    if rc in (N.GX_E_REGEX_SYNTAX, N.GX_E_UNSUPPORTED_CONSTRUCT, N.GX_E_LIMIT):
        # core/Gorp.java:84-90
        raise DefinitionParseException(rc, "Internal error: problem with PolyMatcher construction: " + N.last_error())
    _check(rc)
    return _Handle(h)


class PolyMatcher:
    """core/autom/PolyMatcher.java: multi-pattern matcher over one product DFA."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def create(*patterns, host_only=False, flags=0):
        if len(patterns) == 1 and isinstance(patterns[0], (list, tuple)):
            patterns = list(patterns[0])
        return PolyMatcher(_create(list(patterns), None, flags | (N.GX_CREATE_HOST_ONLY if host_only else 0)))

    def match(self, s):
        """Indexes of all patterns that matched (ascending); [] when none."""
        a = _utf16(s)
        cap = max(1, N.lib().gx_num_extractions(self._h.ptr))
        out = np.zeros(cap, np.int32)
        c = N.lib().gx_match_one_utf16(self._h.ptr, a.ctypes.data if len(a) else None, len(a), out.ctypes.data, cap)
        if c < 0:
            raise GorpError(-c, N.last_error())
        return out[:c].tolist()

    def match_batch(self, data, offsets):
        """PolyMatcher.match for every line of a CSR batch: list of index lists (gx_match_batch + gx_state_accepts)."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets)
        n = len(offsets) - 1
        first = np.zeros(n, np.int32)
        states = np.zeros(n, np.int32)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.offsets64 = 1 if offsets.dtype == np.uint64 else 0
        _check(N.lib().gx_match_batch(self._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, first.ctypes.data,
                                      states.ctypes.data, C.byref(o)))
        cap = max(1, N.lib().gx_num_extractions(self._h.ptr))
        buf = np.zeros(cap, np.int32)
        cache = {}
        out = []
        for st in states.tolist():
            if st not in cache:
                c = N.lib().gx_state_accepts(self._h.ptr, st, buf.ctypes.data, cap)
                cache[st] = buf[:c].tolist()
            out.append(cache[st])
        return out

    def stat(self, which):
        return N.lib().gx_stat(self._h.ptr, which)


class Gorp:
    """core/Gorp.java: processor built from a definition; extract() one line or a batch."""

    def __init__(self, handle, extractions):
        self._h = handle
        self._matcher = PolyMatcher(handle)
        self._extractions = extractions
        for x in extractions:
            x._gorp_handle = handle
        self._meta_sent = False

    def _send_meta(self):
        """gx_set_extraction_meta for handles built from regex strings (names live on this side)."""
        if self._meta_sent:
            return
        import json
        for k, x in enumerate(self._extractions):
            names = [s.encode("utf-8") for s in x._extractorNames]
            arr = (C.c_char_p * max(1, len(names)))(*names)
            app = json.dumps(x.getExtra(), ensure_ascii=False).encode("utf-8") if x.getExtra() else None
            _check(N.lib().gx_set_extraction_meta(self._h.ptr, k, x.getName().encode("utf-8"), arr, len(names), app))
        self._meta_sent = True

    def results_to_jsonl(self, data, offsets, match_id, caps, id_as=None, utf8_passthrough=False, want_line_offsets=False):
        """gx_results_to_jsonl on host buffers: asMap(id_as) of every matched line as JSON Lines (bytes)."""
        self._send_meta()
        data = np.ascontiguousarray(data, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets)
        match_id = np.ascontiguousarray(match_id, dtype=np.int32)
        caps = np.ascontiguousarray(caps, dtype=np.int32)
        n = len(offsets) - 1
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.offsets64 = 1 if offsets.dtype == np.uint64 else 0
        o.utf8_passthrough = 1 if utf8_passthrough else 0
        ida = id_as.encode("utf-8") if id_as is not None else None
        size = C.c_uint64(0)
        args = (self._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n, match_id.ctypes.data if n else None,
                caps.ctypes.data if caps.size else None, ida)
        _check(N.lib().gx_results_to_jsonl(*args, None, 0, C.byref(size), None, C.byref(o)))
        out = np.zeros(max(1, size.value), np.uint8)
        loff = np.zeros(n + 1, np.uint64)
        _check(N.lib().gx_results_to_jsonl(*args, out.ctypes.data, size.value, C.byref(size), loff.ctypes.data, C.byref(o)))
        text = out[:size.value].tobytes()
        return (text, loff) if want_line_offsets else text

    def text_to_jsonl(self, text, id_as=None, utf8_passthrough=False, utf8=False):
        """gx_text_to_jsonl on a host buffer: raw log text -> JSON Lines of the matched lines.
        utf8: the text is UTF-8 and is matched as the decoded Strings (gx_batch_opts.utf8 = 1; implies utf8_passthrough).
        Returns (jsonl bytes, n_lines, n_matched, n_exceptions)."""
        self._send_meta()
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.utf8_passthrough = 1 if utf8_passthrough else 0
        o.utf8 = 1 if utf8 else 0
        ida = id_as.encode("utf-8") if id_as is not None else None
        size, nl, nm, nx = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        ptr = raw.ctypes.data if raw.size else None
        _check(N.lib().gx_text_to_jsonl(self._h.ptr, ptr, raw.size, ida, None, 0, C.byref(size), C.byref(nl), C.byref(nm), C.byref(nx), C.byref(o)))
        out = np.zeros(max(1, size.value), np.uint8)
        _check(N.lib().gx_text_to_jsonl(self._h.ptr, ptr, raw.size, ida, out.ctypes.data, size.value, C.byref(size), C.byref(nl), C.byref(nm),
                                        C.byref(nx), C.byref(o)))
        return out[:size.value].tobytes(), nl.value, nm.value, nx.value

    def text_to_jsonl_device(self, text_ptr, size, out_ptr, out_cap, id_as=None, utf8_passthrough=False, stream=None, utf8=False):
        """gx_text_to_jsonl on device buffers (ints); out_ptr=None only asks for the size.
        Returns (text size, n_lines, n_matched, n_exceptions)."""
        self._send_meta()
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1
        o.utf8_passthrough = 1 if utf8_passthrough else 0
        o.utf8 = 1 if utf8 else 0
        o.stream = stream
        size_out, nl, nm, nx = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_text_to_jsonl(self._h.ptr, text_ptr, size, id_as.encode("utf-8") if id_as is not None else None, out_ptr, out_cap,
                                        C.byref(size_out), C.byref(nl), C.byref(nm), C.byref(nx), C.byref(o)))
        return size_out.value, nl.value, nm.value, nx.value

    def results_to_jsonl_device(self, data_ptr, offsets_ptr, n, match_id_ptr, caps_ptr, out_ptr, out_cap, line_offsets_ptr=None,
                                id_as=None, offsets64=False, utf8_passthrough=False, stream=None):
        """Device pointers; returns the size of the text (out_ptr=None only asks for it)."""
        self._send_meta()
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1
        o.offsets64 = 1 if offsets64 else 0
        o.utf8_passthrough = 1 if utf8_passthrough else 0
        o.stream = stream
        size = C.c_uint64(0)
        _check(N.lib().gx_results_to_jsonl(self._h.ptr, data_ptr, offsets_ptr, n, match_id_ptr, caps_ptr,
                                           id_as.encode("utf-8") if id_as is not None else None, out_ptr, out_cap, C.byref(size),
                                           line_offsets_ptr, C.byref(o)))
        return size.value

    # -- construction ------------------------------------------------------
    @staticmethod
    def construct(extractions, cooker=None, host_only=False, flags=0):
        """Gorp.construct(defs, cooker) (core/Gorp.java:50-92).  extractions: list of FlattenedExtraction (what
        CookedDefinitions.getExtractions() yields); cooker: an ExtractionCooker, default HipExtractionCooker.
        flags: GX_CREATE_* kernel-choice bits (measurements and tests; results never depend on them)."""
        cooker = cooker or HipExtractionCooker.instance()
        autom, regexps, cooked = [], [], []
        for i, ext in enumerate(extractions):
            a, r, _ = ext.build(cooker)
            autom.append(a)
            regexps.append(r)
            cooked.append(cooker.cook(len(cooked), r, ext))
        h = _create(autom, regexps, flags | (N.GX_CREATE_HOST_ONLY if host_only else 0))
        return Gorp(h, cooked)

    @staticmethod
    def from_blob(blob, extractions, host_only=False, flags=0):
        """Rebuild on another rank from the broadcast table blob (no recompilation)."""
        b = np.frombuffer(bytes(blob), dtype=np.uint8)
        h = C.c_void_p()
        _check(N.lib().gx_create_from_blob(b.ctypes.data, len(b), flags | DEFAULT_CREATE_FLAGS | (N.GX_CREATE_HOST_ONLY if host_only else 0), C.byref(h)))
        return Gorp(_Handle(h), extractions)

    def blob(self):
        n = N.lib().gx_blob_size(self._h.ptr)
        out = np.zeros(n, np.uint8)
        _check(N.lib().gx_blob_copy(self._h.ptr, out.ctypes.data, n))
        return out

    def getExtractions(self):
        return list(self._extractions)

    def getMatcher(self):
        return self._matcher

    @property
    def max_groups(self):
        return N.lib().gx_max_groups(self._h.ptr)

    def num_groups(self, k):
        return N.lib().gx_num_groups(self._h.ptr, k)

    def stat(self, which):
        return N.lib().gx_stat(self._h.ptr, which)

    # -- per-line API (core/Gorp.java:145-186) -------------------------------
    def extract(self, input_line, allowFallbacks=False):
        a = _utf16(input_line)
        mid = C.c_int32(0)
        caps = np.full(max(2 * self.max_groups, 1), -1, np.int32)
        _check(N.lib().gx_extract_one_utf16(self._h.ptr, a.ctypes.data if len(a) else None, len(a), C.byref(mid),
                                            caps.ctypes.data))
        return self._materialise(input_line, mid.value, caps, allowFallbacks, units=a)

    def extractSafe(self, input_line):
        return self.extract(input_line, True)

    def _materialise(self, line, match_id, caps, allowFallbacks=False, units=None):
        """units: the line's UTF-16 code units when the capture offsets count those (one-String API: a character
        outside the BMP is two units, so the offsets are not indexes into the Python str)."""
        if match_id == -1:
            return None
        if match_id <= -2:
            k = -2 - match_id
            extr = self._extractions[k]
            if allowFallbacks:
                return None  # core/Gorp.java:178-185 retries the same extraction, then gives up
            raise ExtractionException(line, "Internal error: high-level match for extraction #%d (%s) failed to match "
                                            "generated regexp: %s" % (k, extr.getName(), extr.getRegexpDesc()))
        extr = self._extractions[match_id]
        values = []
        for g in range(self.num_groups(match_id)):
            b, e = int(caps[2 * g]), int(caps[2 * g + 1])
            if b < 0:
                values.append(None)
            elif units is not None:
                values.append(units[b:e].tobytes().decode("utf-16-le", "surrogatepass"))
            else:
                values.append(line[b:e])
        return ExtractionResult(extr.getName(), line, extr, extr._extractorNames, values)

    # -- batch API -----------------------------------------------------------
    def extract_batch(self, data, offsets, match_only=False, strip_eol=False, kernel=0, line_bytes_hint=0, compact=False, uneven=0, utf8=None,
                      utf8_line_flags=None):
        """Host buffers: data uint8[total] (Latin-1 code units) or uint16[total] (UTF-16 code units),
        offsets uint32|uint64[n+1] in code units.
        Returns (match_id int32[n], caps int32[n, 2*max_groups]); with compact=True (or 1) the compact rows
        uint16[n, 1 + 2*max_groups] and the number of offsets that did not fit them (see unpack_rows); with compact=2
        the u8 rows uint8[n, 1 + 2*max_groups] (lines shorter than 255 bytes, at most 126 extractions).
        kernel: GX_KERNEL_* (0 = the library chooses).
        utf8: None: a byte is a Latin-1 code unit; "bytes" / "units": the lines are UTF-8 and are matched as the Strings Java
        would see, capture offsets in bytes of the line / in UTF-16 code units of the String (gx_batch_opts.utf8 = 1 / 2).
        utf8_line_flags: uint8[n], the flags split_lines(want_flags=True) gave for these lines (saves a sweep)."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        n = len(offsets) - 1
        mid = np.zeros(n, np.int32)
        caps = np.full((n, 2 * self.max_groups), -1, np.int32)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.offsets64 = 1 if offsets.dtype == np.uint64 else 0
        o.match_only = 1 if match_only else 0
        o.strip_eol = 1 if strip_eol else 0
        o.utf16 = 1 if utf16 else 0
        o.kernel = int(kernel) or DEFAULT_KERNEL
        o.line_bytes_hint = int(line_bytes_hint)
        o.uneven_lines = int(uneven)  # gx_batch_opts.uneven_lines: 0 = the library looks at the offsets itself
        o.utf8 = _utf8_mode(utf8)
        if utf8_line_flags is not None:
            utf8_line_flags = np.ascontiguousarray(utf8_line_flags, dtype=np.uint8)
            if len(utf8_line_flags) != n:
                raise ValueError("utf8_line_flags: one flag per line")
            o.utf8_line_flags = utf8_line_flags.ctypes.data if n else None
        if compact and not match_only and self.stat(8):
            rows = np.zeros((n, 1 + 2 * self.max_groups), np.uint8 if int(compact) == 2 else np.uint16)
            over = C.c_uint64(0)
            o.compact_results = int(compact)
            o.overflow = C.cast(C.pointer(over), C.c_void_p)
            _check(N.lib().gx_extract_batch(self._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n,
                                            None, rows.ctypes.data, C.byref(o)))
            return rows, over.value
        _check(N.lib().gx_extract_batch(self._h.ptr, data.ctypes.data if data.size else None, offsets.ctypes.data, n,
                                        mid.ctypes.data, caps.ctypes.data if caps.size else None, C.byref(o)))
        return mid, caps

    def extract_batch_device(self, data_ptr, offsets_ptr, n, match_id_ptr, caps_ptr, offsets64=False, match_only=False,
                             stream=None, no_sync=False, strip_eol=False, line_bytes_hint=0, kernel=0, compact=False,
                             overflow_ptr=None, uneven=0, max_line_bytes=0, utf16=False, utf8=0, utf8_line_flags_ptr=None):
        """Device pointers (ints), e.g. torch tensors' data_ptr(); results stay in HBM.  line_bytes_hint sizes
        the kernel's staging area (0: 200 bytes with no_sync, else the batch's mean line length).
        max_line_bytes: the caller's promise that no line is longer (gx_batch_opts.max_line_bytes: no follow-up launch).
        compact=True: caps_ptr receives compact rows uint16[n, 1 + 2*max_groups] (match_id_ptr may be None),
        overflow_ptr (device uint64, zeroed by the caller) counts the offsets that did not fit.
        utf8: gx_batch_opts.utf8 (0, 1 = "bytes", 2 = "units"); utf8_line_flags_ptr: the device flags of split_lines_device."""
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1
        o.offsets64 = 1 if offsets64 else 0
        o.match_only = 1 if match_only else 0
        o.stream = stream
        o.no_sync = 1 if no_sync else 0
        o.strip_eol = 1 if strip_eol else 0
        o.line_bytes_hint = int(line_bytes_hint)
        o.kernel = int(kernel) or DEFAULT_KERNEL
        o.compact_results = int(compact)   # 1 / True: u16 rows; 2: u8 rows
        o.overflow = overflow_ptr
        o.uneven_lines = int(uneven)  # 2: lines differ much in length (0 with a hint or no_sync: taken as 1, similar lengths)
        o.max_line_bytes = int(max_line_bytes)
        o.utf16 = 1 if utf16 else 0
        o.utf8 = _utf8_mode(utf8)
        o.utf8_line_flags = utf8_line_flags_ptr
        _check(N.lib().gx_extract_batch(self._h.ptr, data_ptr, offsets_ptr, n, match_id_ptr, caps_ptr, C.byref(o)))

    # -- outcomes of a finished batch (gx_count_outcomes / gx_select_lines / gx_text_select) --------------------------
    @property
    def num_extractions(self):
        return N.lib().gx_num_extractions(self._h.ptr)

    def outcome_index(self, match_id):
        """The outcome index of a match id (include/gorp_hip.h): id in [0, K) -> id; -1 (no match) -> K; -2-k (exception of
        extraction k) -> K + 1 + k; any other value -> 2K + 1.  Scalars or arrays."""
        K = self.num_extractions
        v = np.asarray(match_id, dtype=np.int64)
        out = np.full(v.shape, 2 * K + 1, np.int64)
        hit = (v >= 0) & (v < K)
        out[hit] = v[hit]
        out[v == -1] = K
        exc = (v <= -2) & (v >= -1 - K)
        out[exc] = K + 1 + (-2 - v[exc])
        return int(out) if out.ndim == 0 else out

    def want_mask(self, want):
        """uint8[2K + 1] over the outcome index from a byte mask of that length, or from names: "unmatched", "exceptions" (of every
        extraction), an extraction's name or index (its matched lines) -- one of them or a list."""
        K = self.num_extractions
        if isinstance(want, (bytes, bytearray, np.ndarray)):
            mask = np.ascontiguousarray(np.frombuffer(want, dtype=np.uint8) if isinstance(want, (bytes, bytearray)) else want, dtype=np.uint8)
            if mask.shape != (2 * K + 1,):
                raise ValueError("want mask must have 2K + 1 = %d entries" % (2 * K + 1))
            return mask
        mask = np.zeros(2 * K + 1, np.uint8)
        names = [x.getName() for x in self._extractions]
        for w in ([want] if isinstance(want, (str, int, np.integer)) else list(want)):
            if isinstance(w, (int, np.integer)) and not isinstance(w, bool):
                if not 0 <= int(w) < K:
                    raise ValueError("no extraction %d" % int(w))
                mask[int(w)] = 1
            elif w == "unmatched":
                mask[K] = 1
            elif w == "exceptions":
                mask[K + 1:] = 1
            elif w in names:
                mask[names.index(w)] = 1
            else:
                raise ValueError("unknown outcome %r" % (w,))
        return mask

    def _ids_format(self, ids):
        """compact_results value of an id column given as a numpy array: int32[n] -> 0, uint16 rows -> 1, uint8 rows -> 2."""
        if ids.dtype == np.int32 and ids.ndim == 1:
            return 0
        if ids.dtype in (np.uint16, np.uint8) and ids.ndim == 2 and ids.shape[1] == 1 + 2 * self.max_groups:
            return 1 if ids.dtype == np.uint16 else 2
        raise TypeError("ids: int32[n], or result rows uint16|uint8[n, 1 + 2*max_groups]")

    def count_outcomes(self, ids):
        """gx_count_outcomes on a host array (int32 match ids, or u16 / u8 result rows): uint64[2K + 2] lines per outcome index."""
        ids = np.ascontiguousarray(ids)
        return self.count_outcomes_device(ids.ctypes.data if ids.size else None, len(ids), compact=self._ids_format(ids), device_pointers=False)

    def count_outcomes_device(self, ids_ptr, n, compact=0, stream=None, device_pointers=True):
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.compact_results = int(compact)
        o.stream = stream
        _check(N.lib().gx_count_outcomes(self._h.ptr, ids_ptr, n, counts.ctypes.data, C.byref(o)))
        return counts

    def select_lines(self, data, offsets, ids, rows=None, want="unmatched"):
        """gx_select_lines on host buffers: the lines of the CSR batch (data uint8 or uint16 code units, offsets uint32|uint64)
        whose outcome `want` names (want_mask), in input order.  ids: int32 match ids (rows: their dense capture rows, optional) or
        u16 / u8 result rows.  Returns (index uint32, data, offsets) and, with dense rows given, (.., match_id, caps); with compact
        rows as ids, (.., rows)."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        n = len(offsets) - 1
        mask = self.want_mask(want)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        args = dict(offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False)
        # one pass: no selection is larger than its input, so outputs of the input's size always do
        total = int(offsets[n] - offsets[0]) if n else 0
        index = np.zeros(n, np.uint32)
        out = np.zeros(total, data.dtype)
        out_off = np.zeros(n + 1, offsets.dtype)
        out_ids = np.zeros(ids.shape, ids.dtype)
        out_caps = None if caps is None else np.zeros((n, 2 * self.max_groups), np.int32)
        # (numpy gives an empty array an address too: every output is asked for, whatever its size)
        k, nbytes = self.select_lines_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), mask, out_index_ptr=index.ctypes.data,
                                             out_data_ptr=out.ctypes.data, out_offsets_ptr=out_off.ctypes.data, out_ids_ptr=out_ids.ctypes.data,
                                             out_caps_ptr=None if out_caps is None else out_caps.ctypes.data, cap_lines=n,
                                             out_bytes_cap=total * data.itemsize, **args)
        index, out, out_off, out_ids = index[:k], out[:nbytes // data.itemsize], out_off[:k + 1], out_ids[:k]
        out_caps = None if out_caps is None else out_caps[:k]
        if compact:
            return index, out, out_off, out_ids
        if caps is not None:
            return index, out, out_off, out_ids, out_caps
        return index, out, out_off

    def select_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, want, out_index_ptr=None, out_data_ptr=None,
                            out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0, offsets64=False,
                            utf16=False, compact=0, stream=None, no_sync=False, device_pointers=True):
        """gx_select_lines on device pointers (ints); every output optional, none at all only asks for the sizes.
        Returns (lines selected, bytes selected).  GorpError with code GX_E_LIMIT when a capacity is too small."""
        mask = self.want_mask(want)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.compact_results = int(compact)
        o.stream = stream
        o.no_sync = 1 if no_sync else 0
        k, nbytes = C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_select_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, mask.ctypes.data, out_index_ptr, out_data_ptr,
                                       out_offsets_ptr, out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap, C.byref(k), C.byref(nbytes), C.byref(o)))
        return k.value, nbytes.value

    # -- lines by the values they captured (gx_select_lines_where / gx_text_select_where) ---------------------------------
    _WHERE_OPS = {"set": (N.GX_WHERE_SET, 0), "unset": (N.GX_WHERE_SET, 1), "==": (N.GX_WHERE_EQ, 0), "!=": (N.GX_WHERE_EQ, 1),
                  "startswith": (N.GX_WHERE_PREFIX, 0), "endswith": (N.GX_WHERE_SUFFIX, 0), "contains": (N.GX_WHERE_CONTAINS, 0),
                  "not contains": (N.GX_WHERE_CONTAINS, 1), "<": (N.GX_WHERE_INT_LT, 0), "<=": (N.GX_WHERE_INT_LE, 0),
                  ">": (N.GX_WHERE_INT_GT, 0), ">=": (N.GX_WHERE_INT_GE, 0)}

    def where_terms(self, spec, units="latin-1"):
        """Resolves a list of (extraction, extractor, op, value) -- value may be left out for "set" / "unset" -- into gx_where_term
        records: extraction is a name or an index, extractor a name or a group index (a name two groups of the extraction share is a
        ValueError), op one of "set", "unset", "==", "!=", "startswith", "endswith", "contains", "not contains", "<", "<=", ">",
        ">=".  An int value selects the integer form of == / != (the group's number format: set_number_format; Long.parseLong's
        rule for ASCII input by default); a str is encoded to the batch's code units (units: "latin-1" bytes, "utf-8" bytes or
        "utf-16" units), bytes are taken as they are.  The number of "<", "<=", ">", ">=" may be a str where the group has a number
        format other than "long": it is converted by parse_number under that format (GorpError if it is no number).  Returns
        (ctypes array, number of terms, what keeps the literals alive); a WhereTerms passes through."""
        if isinstance(spec, WhereTerms):
            return spec
        if units not in ("latin-1", "utf-8", "utf-16"):
            raise ValueError("units: latin-1, utf-8 or utf-16")
        names = [x.getName() for x in self._extractions]
        spec = list(spec)
        arr = (N.gx_where_term * max(1, len(spec)))()
        keep = []
        for t, item in enumerate(spec):
            item = tuple(item)
            if len(item) == 3:
                item = item + (None,)
            if len(item) != 4:
                raise ValueError("a term is (extraction, extractor, op, value)")
            ex, group, op, value = item
            if isinstance(ex, (int, np.integer)) and not isinstance(ex, bool):
                if not 0 <= int(ex) < len(names):
                    raise ValueError("no extraction %d" % int(ex))
                k = int(ex)
            elif ex in names:
                k = names.index(ex)
            else:
                raise ValueError("unknown extraction %r" % (ex,))
            groups = list(self._extractions[k]._extractorNames)
            if isinstance(group, (int, np.integer)) and not isinstance(group, bool):
                if not 0 <= int(group) < self.num_groups(k):
                    raise ValueError("extraction %r has no group %d" % (names[k], int(group)))
                g = int(group)
            elif groups.count(group) == 1:
                g = groups.index(group)
            elif groups.count(group) > 1:
                raise ValueError("extractor name %r is shared by %d groups of %r: name the group by its index" % (group, groups.count(group), names[k]))
            else:
                raise ValueError("extraction %r has no extractor %r" % (names[k], group))
            if op not in self._WHERE_OPS:
                raise ValueError("unknown op %r" % (op,))
            code, negate = self._WHERE_OPS[op]
            m = arr[t]
            m.extraction, m.group, m.negate = k, g, negate
            if code == N.GX_WHERE_SET:
                if value is not None:
                    raise ValueError("%r takes no value" % op)
            elif isinstance(value, (int, np.integer)) and not isinstance(value, bool):
                if code == N.GX_WHERE_EQ:
                    code = N.GX_WHERE_INT_EQ
                elif code < N.GX_WHERE_INT_EQ:
                    raise ValueError("%r takes text, not a number" % op)
                if not -2 ** 63 <= int(value) < 2 ** 63:
                    raise ValueError("a number must fit int64")
                m.number = int(value)
            elif isinstance(value, str) and code >= N.GX_WHERE_INT_EQ and self.number_format(k, g)[0] != "long":
                # (a group with a number format of its own: the str is a number in that format, "2026-01-03T00:00:00Z")
                kind, scale = self.number_format(k, g)
                number = parse_number(kind, scale, value)
                if number is None:
                    raise GorpError(N.GX_E_ARG, "%r is no number under %s(%d), the format of %r group %d" % (value, kind, scale, names[k], g))
                m.number = number
            elif isinstance(value, (str, bytes, bytearray)):
                if code >= N.GX_WHERE_INT_EQ:
                    raise ValueError("%r takes an int" % op)
                if isinstance(value, str):
                    lit = np.frombuffer(value.encode("utf-16-le"), dtype=np.uint16).copy() if units == "utf-16" else np.frombuffer(value.encode(units), dtype=np.uint8).copy()
                elif units == "utf-16":
                    raise ValueError("a utf-16 batch takes str literals")
                else:
                    lit = np.frombuffer(bytes(value), dtype=np.uint8).copy()
                if lit.size > 255:
                    raise ValueError("a literal has at most 255 code units")
                keep.append(lit)
                m.text = lit.ctypes.data if lit.size else None
                m.text_units = lit.size
            else:
                raise ValueError("%r needs a value (str, bytes or int)" % op)
            m.op = code
        return WhereTerms(arr, len(spec), keep, units)

    def _where_want(self, terms, want):
        if isinstance(want, str) and want == "matched-by-terms":
            mask = np.zeros(2 * self.num_extractions + 1, np.uint8)
            for t in range(terms.n):
                mask[terms.array[t].extraction] = 1
            return mask
        return self.want_mask(want)

    def select_lines_where(self, data, offsets, ids, rows, where, want="matched-by-terms", utf8=None):
        """gx_select_lines_where on host buffers: select_lines, and of the lines of an extraction that has terms only those on which
        every term holds.  where: a list of (extraction, extractor, op, value) (where_terms).  want: as select_lines takes it; the
        default marks exactly the extractions that have terms.  utf8="bytes": the batch is UTF-8 with byte offsets
        (extract_batch(utf8="bytes")) and str literals are encoded as UTF-8.  Returns what select_lines returns."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are compared in the units the offsets count)')
        terms = self.where_terms(where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        n = len(offsets) - 1
        mask = self._where_want(terms, want)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        args = dict(offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8))
        total = int(offsets[n] - offsets[0]) if n else 0
        index = np.zeros(n, np.uint32)
        out = np.zeros(total, data.dtype)
        out_off = np.zeros(n + 1, offsets.dtype)
        out_ids = np.zeros(ids.shape, ids.dtype)
        out_caps = None if caps is None else np.zeros((n, 2 * self.max_groups), np.int32)
        k, nbytes = self.select_lines_where_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), mask, terms, out_index_ptr=index.ctypes.data,
                                                   out_data_ptr=out.ctypes.data, out_offsets_ptr=out_off.ctypes.data, out_ids_ptr=out_ids.ctypes.data,
                                                   out_caps_ptr=None if out_caps is None else out_caps.ctypes.data, cap_lines=n,
                                                   out_bytes_cap=total * data.itemsize, **args)
        index, out, out_off, out_ids = index[:k], out[:nbytes // data.itemsize], out_off[:k + 1], out_ids[:k]
        out_caps = None if out_caps is None else out_caps[:k]
        if compact:
            return index, out, out_off, out_ids
        if caps is not None:
            return index, out, out_off, out_ids, out_caps
        return index, out, out_off

    def select_lines_where_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, want, where, out_index_ptr=None, out_data_ptr=None,
                                  out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0, offsets64=False,
                                  utf16=False, compact=0, stream=None, no_sync=False, device_pointers=True, utf8=False):
        """gx_select_lines_where on device pointers (ints), select_lines_device with terms (where_terms' result, or its input: then
        str literals are encoded for the batch utf16 / utf8 name).  Returns (lines selected, bytes selected)."""
        terms = self.where_terms(where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        mask = self._where_want(terms, want)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        o.no_sync = 1 if no_sync else 0
        k, nbytes = C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_select_lines_where(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, mask.ctypes.data, terms.array, terms.n, out_index_ptr,
                                             out_data_ptr, out_offsets_ptr, out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap, C.byref(k), C.byref(nbytes),
                                             C.byref(o)))
        return k.value, nbytes.value

    def text_select_where(self, text, where, want="matched-by-terms", utf8=False):
        """gx_text_select_where on a host buffer: text_select with terms.  Returns (selected text bytes, counts uint64[2K + 2] --
        of outcomes, whatever the terms say --, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        ptr = raw.ctypes.data if raw.size else None
        out = np.zeros(max(1, raw.size), np.uint8)
        size, counts, n_lines = self.text_select_where_device(ptr, raw.size, want, where, out.ctypes.data, raw.size, device_pointers=False, utf8=utf8)
        return out[:size].tobytes(), counts, n_lines

    def text_select_where_device(self, text_ptr, size, want, where, out_ptr, out_cap, stream=None, device_pointers=True, utf8=False):
        """gx_text_select_where on device buffers (ints); out_ptr=None only asks for the sizes.  Returns (selected bytes, counts, n_lines)."""
        terms = self.where_terms(where, units="utf-8" if utf8 else "latin-1")
        mask = self._where_want(terms, want)
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out_size, nl = C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_text_select_where(self._h.ptr, text_ptr, size, mask.ctypes.data, terms.array, terms.n, out_ptr, out_cap, C.byref(out_size),
                                            counts.ctypes.data, C.byref(nl), C.byref(o)))
        return out_size.value, counts, nl.value

    # -- captured numbers, summarised (gx_capture_stats / gx_text_capture_stats) -------------------------------------------
    def _extraction_and_group(self, ex, group):
        """(k, g) of an extraction given by name or index and one of its groups given by extractor name or index."""
        names = [x.getName() for x in self._extractions]
        if isinstance(ex, (int, np.integer)) and not isinstance(ex, bool):
            if not 0 <= int(ex) < len(names):
                raise ValueError("no extraction %d" % int(ex))
            k = int(ex)
        elif ex in names:
            k = names.index(ex)
        else:
            raise ValueError("unknown extraction %r" % (ex,))
        groups = list(self._extractions[k]._extractorNames)
        if isinstance(group, (int, np.integer)) and not isinstance(group, bool):
            if not 0 <= int(group) < self.num_groups(k):
                raise ValueError("extraction %r has no group %d" % (names[k], int(group)))
            return k, int(group)
        if groups.count(group) == 1:
            return k, groups.index(group)
        if groups.count(group) > 1:
            raise ValueError("extractor name %r is shared by %d groups of %r: name the group by its index" % (group, groups.count(group), names[k]))
        raise ValueError("extraction %r has no extractor %r" % (names[k], group))

    # -- how a group is read as a number (gx_set_number_format) ----------------------------------------------------------
    def set_number_format(self, extraction, group, kind, scale=0):
        """gx_set_number_format: from now on every call that parses this group as a number -- where_terms' integer comparisons,
        capture_stats, the value group of group_lines / group_quantiles / top_groups / top_lines / capture_quantiles, both groups of
        bucket_lines -- reads it as
        kind "long" (Long.parseLong, the default), "decimal" (scale 0 .. 18: the value times 10^scale, cut toward zero), "iso8601" or
        "clf" (scale 0, 3, 6 or 9: the instant in 10^-scale seconds since the epoch).  extraction and group are resolved as
        where_terms resolves them.  Needs no device; not kept in the blob."""
        k, g = self._extraction_and_group(extraction, group)
        if kind not in NUMBER_KINDS:
            raise ValueError("kind: long, decimal, iso8601 or clf")
        if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 0 <= int(scale) < 2 ** 32:
            raise ValueError("scale: a non-negative int")
        f = N.gx_number_format(NUMBER_KINDS.index(kind), int(scale))
        _check(N.lib().gx_set_number_format(self._h.ptr, k, g, C.byref(f)))

    def number_format(self, extraction, group):
        """(kind, scale) of the group: gx_get_number_format."""
        k, g = self._extraction_and_group(extraction, group)
        f = N.gx_number_format()
        _check(N.lib().gx_get_number_format(self._h.ptr, k, g, C.byref(f)))
        return NUMBER_KINDS[f.kind], int(f.scale)

    def measures(self, spec):
        """Resolves a list of (extraction, extractor) or (extraction, extractor, edges) into gx_measure records: extraction is a name or
        an index, extractor a name or a group index (a name two groups of the extraction share is a ValueError), edges an optional
        strictly ascending list of at most 64 int64 histogram edges.  At most 64 measures and 1 024 edges in all.  Returns a Measures
        (which keeps the edge arrays alive); a Measures passes through."""
        if isinstance(spec, Measures):
            return spec
        spec = list(spec)
        if len(spec) > 64:
            raise ValueError("at most 64 measures")
        arr = (N.gx_measure * max(1, len(spec)))()
        keep = []
        for t, item in enumerate(spec):
            item = tuple(item)
            if len(item) == 2:
                item = item + (None,)
            if len(item) != 3:
                raise ValueError("a measure is (extraction, extractor[, edges])")
            k, g = self._extraction_and_group(item[0], item[1])
            raw = [] if item[2] is None else list(item[2])
            if any(isinstance(e, bool) or not isinstance(e, (int, np.integer)) for e in raw):
                raise ValueError("edges are ints")
            if any(not -2 ** 63 <= int(e) < 2 ** 63 for e in raw):
                raise ValueError("an edge must fit int64")
            edges = np.array([int(e) for e in raw], dtype=np.int64)
            if edges.size > 64:
                raise ValueError("a measure has at most 64 edges")
            if edges.size > 1 and not (edges[1:] > edges[:-1]).all():
                raise ValueError("edges must be strictly ascending")
            keep.append(edges)
            m = arr[t]
            m.extraction, m.group, m.n_edges = k, g, edges.size
            m.edges = edges.ctypes.data if edges.size else None
        if sum(e.size for e in keep) > 1024:
            raise ValueError("at most 1024 edges in all")
        return Measures(arr, len(spec), keep)

    @staticmethod
    def _stats_result(measures, stats, hist):
        out, at = [], 0
        for t in range(measures.n):
            s = stats[t]
            bins = measures.array[t].n_edges + 1
            out.append({"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                        "min": s.min if s.numbers else None, "max": s.max if s.numbers else None, "sum": (s.sum_hi << 64) + s.sum_lo,
                        "hist": hist[at:at + bins].copy()})
            at += bins
        return out

    def capture_stats(self, data, offsets, ids, rows, measures, where=None, utf8=None):
        """gx_capture_stats on host buffers: per measure (measures: Gorp.measures or its input) the lines of its extraction on which
        every term of `where` holds (where_terms; None: all of them), classed by what the group captured.  data / offsets / ids / rows
        and utf8 as select_lines_where takes them.  Returns one dict per measure: lines, numbers, unset, not_numbers, min, max (None
        without a number), sum (exact, a Python int) and hist (uint64[n_edges + 1])."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        return self.capture_stats_device(ptr(data), offsets.ctypes.data, len(offsets) - 1, ptr(ids), ptr(caps), measures, where,
                                         offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8))

    def capture_stats_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, measures, where=None, offsets64=False, utf16=False, compact=0,
                             stream=None, device_pointers=True, utf8=False):
        """gx_capture_stats on device pointers (ints).  Returns what capture_stats returns."""
        measures = self.measures(measures)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        stats = (N.gx_measure_stats * max(1, measures.n))()
        hist = np.zeros(measures.n_bins, np.uint64)
        _check(N.lib().gx_capture_stats(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, measures.array, measures.n, terms.array, terms.n, stats,
                                        hist.ctypes.data, C.byref(o)))
        return self._stats_result(measures, stats, hist)

    def text_capture_stats(self, text, measures, where=None, utf8=False):
        """gx_text_capture_stats on a host buffer: raw text -> lines -> extraction -> capture_stats.  Returns (the list capture_stats
        returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        return self.text_capture_stats_device(raw.ctypes.data if raw.size else None, raw.size, measures, where, device_pointers=False, utf8=utf8)

    def text_capture_stats_device(self, text_ptr, size, measures, where=None, stream=None, device_pointers=True, utf8=False):
        """gx_text_capture_stats on a device buffer (int).  Returns (stats, counts, n_lines)."""
        measures = self.measures(measures)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        stats = (N.gx_measure_stats * max(1, measures.n))()
        hist = np.zeros(measures.n_bins, np.uint64)
        nl = C.c_uint64(0)
        _check(N.lib().gx_text_capture_stats(self._h.ptr, text_ptr, size, measures.array, measures.n, terms.array, terms.n, stats, hist.ctypes.data,
                                             counts.ctypes.data, C.byref(nl), C.byref(o)))
        return self._stats_result(measures, stats, hist), counts, nl.value

    # -- lines grouped by the text they captured (gx_group_lines / gx_text_group_lines) ----------------------------------------
    def group_parts(self, spec):
        """Resolves a list of (extraction, key extractor) or (extraction, key extractor, value extractor) into gx_group_part records:
        extraction is a name or an index, an extractor a name or a group index (a name two groups of the extraction share is a
        ValueError), the value extractor None for a part that only counts.  At most one part per extraction, at most 64 parts.
        Returns a GroupParts; a GroupParts passes through."""
        if isinstance(spec, GroupParts):
            return spec
        spec = list(spec)
        if len(spec) > 64:
            raise ValueError("at most 64 parts")
        arr = (N.gx_group_part * max(1, len(spec)))()
        seen = set()
        for t, item in enumerate(spec):
            item = tuple(item)
            if len(item) == 2:
                item = item + (None,)
            if len(item) != 3:
                raise ValueError("a part is (extraction, key extractor[, value extractor])")
            k, g = self._extraction_and_group(item[0], item[1])
            if k in seen:
                raise ValueError("two parts for extraction %r" % (item[0],))
            seen.add(k)
            arr[t].extraction, arr[t].key_group, arr[t].value_group = k, g, -1 if item[2] is None else self._extraction_and_group(k, item[2])[1]
        return GroupParts(arr, len(spec))

    @staticmethod
    def _group_totals(t):
        return {"n_keys": t.n_keys, "key_units": t.key_units, "lines": t.lines, "keyed": t.keyed, "unset": t.unset, "exact": bool(t.exact)}

    def group_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                           key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, offsets64=False, utf16=False,
                           compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_group_lines on device pointers (ints); the outputs are the caller's buffers, each optional (none at all: the size query;
        max_keys still sizes the table).  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says
        what the outputs need (n_keys, key_units; exact False: the table overflowed, max_keys = n always suffices); every other
        error raises."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        totals = N.gx_group_totals()
        rc = N.lib().gx_group_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n,
                                    N.GX_GROUP_WEAK_HASH if weak_hash else 0, C.byref(out), C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._group_totals(totals)

    def text_group_lines_device(self, text_ptr, size, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None, key_first_line_ptr=None,
                                key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, offsets64=False, stream=None, device_pointers=True,
                                utf8=False, weak_hash=False):
        """gx_text_group_lines on a device buffer (int); outputs as group_lines_device takes them (line_key: one entry per line of the
        text).  Returns (rc, totals, counts, n_lines)."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        totals = N.gx_group_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_lines(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, N.GX_GROUP_WEAK_HASH if weak_hash else 0,
                                         C.byref(out), C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._group_totals(totals), counts, nl.value

    def _group_host(self, call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap, n_q=None):
        """Runs `call(out arrays..., max_keys, key_units_cap)` on host arrays; on GX_E_LIMIT once more with the sizes it reported when
        they are exact, else with the number of lines (which may report exact sizes in turn).  Builds the result dict.  n_q (the
        group_quantiles calls): `call` also takes max_keys x n_q gx_quantile_out rows, and the dict has "quantiles"."""
        max_keys = min(n_lines_cap, 1024) if max_keys is None else max_keys
        key_units_cap = 65536 if key_units_cap is None else key_units_cap
        for attempt in range(3):
            units = np.zeros(max(1, key_units_cap), unit_dtype)
            koff = np.zeros(max_keys + 1, offsets_dtype)
            first = np.zeros(max(1, max_keys), np.uint32)
            lines = np.zeros(max(1, max_keys), np.uint64)
            stats = (N.gx_measure_stats * max(1, max_keys))() if parts.has_values else None
            line_key = np.full(max(1, n_lines_cap), 0xFFFFFFFF, np.uint32)
            rows = None if n_q is None else (N.gx_quantile_out * max(1, max_keys * n_q))()
            got = call(units.ctypes.data, key_units_cap, koff.ctypes.data, first.ctypes.data, lines.ctypes.data, None if stats is None else C.addressof(stats),
                       line_key.ctypes.data, max_keys, *(() if n_q is None else (C.addressof(rows),)))
            rc, totals = got[0], got[1]
            if rc == N.GX_OK:
                break
            if attempt == 2:
                raise GorpError(rc, N.last_error())
            if totals["exact"]:
                max_keys, key_units_cap = max(max_keys, totals["n_keys"]), max(key_units_cap, totals["key_units"])
            else:
                max_keys = n_lines_cap
        k = totals["n_keys"]
        koff, units = koff[:k + 1], units[:totals["key_units"]]
        res = {"key_units": units, "key_offsets": koff, "first_line": first[:k], "lines": lines[:k], "totals": totals, "line_key": line_key,
               "stats": None if stats is None else [{"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                                                      "min": s.min if s.numbers else None, "max": s.max if s.numbers else None,
                                                      "sum": (s.sum_hi << 64) + s.sum_lo} for s in stats[:k]]}
        if n_q is not None:
            res["quantiles"] = [[{"value": r.value if r.rank else None, "rank": r.rank, "below": r.below, "equal": r.equal}
                                 for r in rows[j * n_q:(j + 1) * n_q]] for j in range(k)]
        if keys == "list":
            res["keys"] = [decode(units[int(koff[j]):int(koff[j + 1])]) for j in range(k)]
        elif keys != "csr":
            raise ValueError('keys: "list" or "csr"')
        return res, got[2:]

    def group_lines(self, data, offsets, ids, rows, parts, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None, weak_hash=False):
        """gx_group_lines on host buffers: the lines grouped by the value the part of their extraction names as the key (parts:
        Gorp.group_parts or its input), of the lines on which every term of `where` holds.  data / offsets / ids / rows and utf8 as
        capture_stats takes them.  Returns a dict: keys (a list in order of first appearance: bytes, or str for a UTF-16 batch and
        with utf8; keys="csr": left out), key_units / key_offsets (the same as CSR arrays), first_line, lines (per key), stats (per
        key, a dict as capture_stats gives one without hist; None when no part has a value extractor), line_key (uint32 per input
        line, 0xFFFFFFFF: none) and totals.  On GX_E_LIMIT the call is repeated with the sizes it reported when they are exact; when the
        table itself overflowed, with max_keys = the number of lines, which may in turn report exact sizes: three calls at the most."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.group_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            return self.group_lines_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), parts, where, units, cap, koff, first, lines, stats, line_key, mk,
                                           offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8),
                                           weak_hash=weak_hash)
        res, _ = self._group_host(call, n, parts, data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap)
        res["line_key"] = res["line_key"][:n]
        return res

    def text_group_lines(self, text, parts, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None):
        """gx_text_group_lines on a host buffer: raw text -> lines -> extraction -> group_lines.  Returns (the dict group_lines returns,
        counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.group_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            return self.text_group_lines_device(raw.ctypes.data if raw.size else None, raw.size, parts, where, units, cap, koff, first, lines, stats, line_key, mk,
                                                device_pointers=False, utf8=utf8)
        res, (counts, n_lines) = self._group_host(call, cap_lines, parts, np.uint8, np.uint32, keys, decode, max_keys, key_units_cap)
        res["line_key"] = res["line_key"][:n_lines]
        return res, counts, n_lines

    # -- every key's lines together (gx_lines_by_key / gx_text_lines_by_key) ------------------------------------------------------
    @staticmethod
    def _by_key_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(keys_kept=t.keys_kept, lines_out=t.lines_out, units_out=t.units_out)
        return d

    def lines_by_key_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, min_lines=1, max_lines=None, where=None, key_units_ptr=None,
                            key_units_cap=0, key_offsets_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0,
                            out_index_ptr=None, out_data_ptr=None, out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0,
                            key_out_lines_ptr=None, key_out_units_ptr=None, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True,
                            utf8=False, weak_hash=False, all_digits=False):
        """gx_lines_by_key on device pointers (ints): the lines whose key has min_lines .. max_lines lines (max_lines None: no upper
        bound), ordered by (key number, input line), as a new CSR batch in the caller's buffers, each optional (none of the out_* and
        key_out_*: the size query); the key_* / line_key / max_keys arguments are group_lines_device's and deliver what it would.
        Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says what the outputs need (n_keys,
        key_units, lines_out, units_out; exact False: the table overflowed, max_keys = n always suffices); every other error raises."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_by_key_out(out_index_ptr, out_data_ptr, out_offsets_ptr, out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap, key_out_lines_ptr, key_out_units_ptr)
        totals = N.gx_by_key_totals()
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (N.GX_BY_KEY_ALL_DIGITS if all_digits else 0)
        rc = N.lib().gx_lines_by_key(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, int(min_lines),
                                     0 if max_lines is None else int(max_lines), flags, C.byref(keys), C.byref(out), C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._by_key_totals(totals)

    def text_lines_by_key_device(self, text_ptr, size, parts, min_lines=1, max_lines=None, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                                 key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, out_ptr=None, out_cap=0,
                                 out_offsets_ptr=None, out_index_ptr=None, key_out_lines_ptr=None, key_out_units_ptr=None, offsets64=False, stream=None,
                                 device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_text_lines_by_key on a device buffer (int); outputs as lines_by_key_device takes them (out_offsets: uint32, out_index: line
        numbers of the text, both sized by the size query).  Returns (rc, totals, counts, n_lines)."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        totals = N.gx_by_key_totals()
        nl = C.c_uint64(0)
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (N.GX_BY_KEY_ALL_DIGITS if all_digits else 0)
        rc = N.lib().gx_text_lines_by_key(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, int(min_lines),
                                          0 if max_lines is None else int(max_lines), flags, C.byref(keys), out_ptr, out_cap, out_offsets_ptr, out_index_ptr,
                                          key_out_lines_ptr, key_out_units_ptr, C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._by_key_totals(totals), counts, nl.value

    def lines_by_key(self, data, offsets, match_id, caps, parts, min_lines=1, max_lines=None, where=None, utf8=None, keys="list", max_keys=None,
                     key_units_cap=None, weak_hash=False, all_digits=False):
        """gx_lines_by_key on host buffers: every kept key's lines together -- keys in order of their first line, lines in input order
        inside each (Collectors.groupingBy on a captured text, insertion-ordered).  data / offsets / match_id (ids or compact rows) /
        caps, parts, where, utf8, keys, max_keys as group_lines takes them; a key is kept when it has min_lines .. max_lines lines
        (max_lines None: no upper bound; min_lines=1, max_lines=1: the keys with one line).  Returns group_lines' dict -- every key, kept
        or not -- plus index (input line of every output line), data / offsets (the kept lines as a CSR batch), ids and caps (their ids
        or whole rows; caps None for compact rows or without caps), key_out_lines / key_out_units (uint64[n_keys + 1]: key j's lines are
        output lines key_out_lines[j] .. key_out_lines[j + 1]) and totals with keys_kept, lines_out, units_out besides group_lines'."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(match_id)
        compact = self._ids_format(ids)
        rows = None if caps is None or compact else np.ascontiguousarray(caps, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.group_parts(parts)
        n = len(offsets) - 1
        total = int(offsets[n] - offsets[0]) if n else 0
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())
        got = {}

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            # no regrouping is larger than its input; the two prefixes are per key
            got.update(index=np.zeros(n, np.uint32), data=np.zeros(total, data.dtype), offsets=np.zeros(n + 1, offsets.dtype), ids=np.zeros(ids.shape, ids.dtype),
                       caps=None if rows is None else np.zeros((n, 2 * self.max_groups), np.int32), key_out_lines=np.zeros(mk + 1, np.uint64),
                       key_out_units=np.zeros(mk + 1, np.uint64))
            return self.lines_by_key_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(rows), parts, min_lines, max_lines, where, units, cap, koff, first, lines,
                                            stats, line_key, mk, out_index_ptr=got["index"].ctypes.data, out_data_ptr=got["data"].ctypes.data,
                                            out_offsets_ptr=got["offsets"].ctypes.data, out_ids_ptr=got["ids"].ctypes.data,
                                            out_caps_ptr=None if got["caps"] is None else got["caps"].ctypes.data, cap_lines=n,
                                            out_bytes_cap=total * data.itemsize, key_out_lines_ptr=got["key_out_lines"].ctypes.data,
                                            key_out_units_ptr=got["key_out_units"].ctypes.data, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact,
                                            device_pointers=False, utf8=bool(utf8), weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._group_host(call, n, parts, data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap)
        res["line_key"] = res["line_key"][:n]
        m, k = res["totals"]["lines_out"], res["totals"]["n_keys"]
        res.update(index=got["index"][:m], data=got["data"][:res["totals"]["units_out"]], offsets=got["offsets"][:m + 1], ids=got["ids"][:m],
                   caps=None if got["caps"] is None else got["caps"][:m], key_out_lines=got["key_out_lines"][:k + 1], key_out_units=got["key_out_units"][:k + 1])
        return res

    def text_lines_by_key(self, text, parts, min_lines=1, max_lines=None, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None):
        """gx_text_lines_by_key on a host buffer: raw text -> lines -> extraction -> lines_by_key.  Returns (the dict lines_by_key returns
        without ids and caps: data holds the kept lines' original bytes, offsets (uint32) delimits them, index holds line numbers of
        the text; counts uint64[2K + 2] of outcomes; n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.group_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())
        got = {}

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            got.update(index=np.zeros(cap_lines, np.uint32), data=np.zeros(raw.size, np.uint8), offsets=np.zeros(cap_lines + 1, np.uint32),
                       key_out_lines=np.zeros(mk + 1, np.uint64), key_out_units=np.zeros(mk + 1, np.uint64))
            return self.text_lines_by_key_device(raw.ctypes.data if raw.size else None, raw.size, parts, min_lines, max_lines, where, units, cap, koff, first, lines,
                                                 stats, line_key, mk, out_ptr=got["data"].ctypes.data if raw.size else None, out_cap=raw.size,
                                                 out_offsets_ptr=got["offsets"].ctypes.data, out_index_ptr=got["index"].ctypes.data,
                                                 key_out_lines_ptr=got["key_out_lines"].ctypes.data, key_out_units_ptr=got["key_out_units"].ctypes.data,
                                                 device_pointers=False, utf8=utf8)
        res, (counts, n_lines) = self._group_host(call, cap_lines, parts, np.uint8, np.uint32, keys, decode, max_keys, key_units_cap)
        res["line_key"] = res["line_key"][:n_lines]
        m, k = res["totals"]["lines_out"], res["totals"]["n_keys"]
        res.update(index=got["index"][:m], data=got["data"][:res["totals"]["units_out"]], offsets=got["offsets"][:m + 1],
                   key_out_lines=got["key_out_lines"][:k + 1], key_out_units=got["key_out_units"][:k + 1])
        return res, counts, n_lines

    # -- captured texts looked up in a dictionary of the caller's (gx_lookup_lines / gx_text_lookup_lines) -------------------------
    @staticmethod
    def _lookup_totals(t):
        return {f: getattr(t, f) for f, _ in N.gx_lookup_totals._fields_}

    @staticmethod
    def _lookup_keep(keep):
        if keep is None or keep is False:
            return N.GX_LOOKUP_KEEP_NOTHING
        if isinstance(keep, str):
            if keep not in ("hits", "others"):
                raise ValueError('keep: None, "hits" or "others"')
            return N.GX_LOOKUP_KEEP_HITS if keep == "hits" else N.GX_LOOKUP_KEEP_OTHERS
        return int(keep)

    @staticmethod
    def lookup_entries(entries, unit_dtype=np.uint8, offsets_dtype=np.uint32, encoding="latin-1"):
        """A dictionary for lookup_lines as a CSR pair (units, offsets): from a list of bytes or str (str is encoded: "utf-16-le" for a
        UTF-16 batch, else `encoding`), from a (units, offsets) pair, or from the dict a group_lines(..., keys="csr") call returned.
        The arrays are made contiguous and of the batch's unit and offset types."""
        if isinstance(entries, dict):
            entries = (entries["key_units"], entries["key_offsets"])
        if isinstance(entries, tuple) and len(entries) == 2 and isinstance(entries[1], np.ndarray):
            units = np.ascontiguousarray(entries[0], dtype=unit_dtype)
            offsets = np.ascontiguousarray(entries[1], dtype=offsets_dtype)
            if offsets.ndim != 1 or offsets.size < 1:
                raise ValueError("entry offsets: m + 1 values")
            return units, offsets
        enc = "utf-16-le" if np.dtype(unit_dtype) == np.uint16 else encoding
        raw = [e.encode(enc, "surrogatepass" if enc == "utf-16-le" else "strict") if isinstance(e, str) else bytes(e) for e in entries]
        width = np.dtype(unit_dtype).itemsize
        offsets = np.zeros(len(raw) + 1, offsets_dtype)
        if raw:
            offsets[1:] = np.cumsum([len(r) // width for r in raw])
        return np.frombuffer(b"".join(raw), dtype=unit_dtype).copy(), offsets

    def lookup_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, entry_units_ptr, entry_offsets_ptr, n_entries, keep=None, where=None,
                            line_entry_ptr=None, entry_same_ptr=None, entry_lines_ptr=None, entry_first_line_ptr=None, entry_stats_ptr=None, out_index_ptr=None,
                            out_data_ptr=None, out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0, offsets64=False,
                            utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_lookup_lines on device pointers (ints), nothing copied: the dictionary is the CSR at entry_units_ptr / entry_offsets_ptr
        (n_entries + 1 offsets as wide as the batch's) -- e.g. the key_units / key_offsets a group_lines_device call left on the device.
        The outputs are the caller's buffers, each optional (none at all: the size query).  keep: None, "hits" or "others".  Returns
        (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says what the kept lines need (lines_out,
        units_out); every other error raises."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_lookup_out(line_entry_ptr, entry_same_ptr, entry_lines_ptr, entry_first_line_ptr, entry_stats_ptr, out_index_ptr, out_data_ptr, out_offsets_ptr,
                              out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap)
        totals = N.gx_lookup_totals()
        rc = N.lib().gx_lookup_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, entry_units_ptr,
                                     entry_offsets_ptr, n_entries, self._lookup_keep(keep), N.GX_GROUP_WEAK_HASH if weak_hash else 0, C.byref(out), C.byref(totals),
                                     C.byref(o))
        if not (rc == N.GX_E_LIMIT and (totals.lines_out or totals.units_out)):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._lookup_totals(totals)

    @staticmethod
    def _lookup_result(parts, m, line_entry, same, lines, first, stats, totals):
        return {"line_entry": line_entry, "entry_same": same[:m], "entry_lines": lines[:m], "entry_first_line": first[:m], "totals": totals,
                "entry_stats": None if stats is None else [{"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                                                            "min": s.min if s.numbers else None, "max": s.max if s.numbers else None,
                                                            "sum": (s.sum_hi << 64) + s.sum_lo} for s in stats[:m]]}

    def lookup_lines(self, data, offsets, ids, rows, parts, entries, keep=None, where=None, utf8=None, weak_hash=False):
        """gx_lookup_lines on host buffers: what the lines captured as their part's key, looked up in `entries` (Gorp.lookup_entries'
        input: a list of str or bytes, a (units, offsets) CSR pair, or the dict a group_lines(..., keys="csr") call returned), of the
        lines on which every term of `where` holds.  data / offsets / ids / rows and utf8 as group_lines takes them.  Returns a dict:
        line_entry (uint32 per input line: the lowest entry with the line's key, 0xFFFFFFFE: a miss, 0xFFFFFFFF: none), entry_same,
        entry_lines, entry_first_line (per entry), entry_stats (per entry, a dict as capture_stats gives one without hist; None when no
        part has a value extractor), totals, and with keep ("hits": wanted.contains(v); "others": !blocked.contains(v), unset lines
        included) the kept lines in input order as a batch: index, data, offsets, ids, caps (None for compact rows or without caps)."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.group_parts(parts)
        n = len(offsets) - 1
        eu, eo = self.lookup_entries(entries, data.dtype, offsets.dtype, "utf-8" if utf8 else "latin-1")
        m = len(eo) - 1
        keep = self._lookup_keep(keep)
        total = int(offsets[n] - offsets[0]) if n else 0
        line_entry = np.full(n, 0xFFFFFFFF, np.uint32)
        same, lines, first = np.zeros(max(1, m), np.uint32), np.zeros(max(1, m), np.uint64), np.zeros(max(1, m), np.uint32)
        stats = (N.gx_measure_stats * max(1, m))() if parts.has_values else None
        kept = {}
        if keep:   # no selection is larger than its input
            kept = dict(index=np.zeros(n, np.uint32), data=np.zeros(total, data.dtype), offsets=np.zeros(n + 1, offsets.dtype), ids=np.zeros(ids.shape, ids.dtype),
                        caps=None if caps is None else np.zeros((n, 2 * self.max_groups), np.int32))
        kp = lambda k: kept[k].ctypes.data if kept.get(k) is not None else None
        rc, totals = self.lookup_lines_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), parts, ptr(eu), eo.ctypes.data if m else None, m, keep, where,
                                              line_entry.ctypes.data, same.ctypes.data, lines.ctypes.data, first.ctypes.data,
                                              None if stats is None else C.addressof(stats), kp("index"), kp("data"), kp("offsets"), kp("ids"), kp("caps"),
                                              cap_lines=n, out_bytes_cap=total * data.itemsize, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact,
                                              device_pointers=False, utf8=bool(utf8), weak_hash=weak_hash)
        _check(rc)
        res = self._lookup_result(parts, m, line_entry, same, lines, first, stats, totals)
        if keep:
            k = totals["lines_out"]
            res.update(index=kept["index"][:k], data=kept["data"][:totals["units_out"]], offsets=kept["offsets"][:k + 1], ids=kept["ids"][:k],
                       caps=None if kept["caps"] is None else kept["caps"][:k])
        return res

    def text_lookup_lines(self, text, parts, entries, keep=None, where=None, utf8=False, weak_hash=False):
        """gx_text_lookup_lines on a host buffer: raw text -> lines -> extraction -> lookup_lines.  Returns (the dict lookup_lines returns
        without ids and caps: data holds the kept lines' original bytes, offsets (uint32) delimits them, index holds line numbers of
        the text; counts uint64[2K + 2] of outcomes; n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        eu, eo = self.lookup_entries(entries, np.uint8, np.uint32, "utf-8" if utf8 else "latin-1")
        m = len(eo) - 1
        keep = self._lookup_keep(keep)
        line_entry = np.full(cap_lines, 0xFFFFFFFF, np.uint32)
        same, lines, first = np.zeros(max(1, m), np.uint32), np.zeros(max(1, m), np.uint64), np.zeros(max(1, m), np.uint32)
        stats = (N.gx_measure_stats * max(1, m))() if parts.has_values else None
        index, data, koff = np.zeros(cap_lines, np.uint32), np.zeros(max(1, raw.size), np.uint8), np.zeros(cap_lines + 1, np.uint32)
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.utf8 = 1 if utf8 else 0
        out = N.gx_lookup_out(line_entry.ctypes.data, same.ctypes.data, lines.ctypes.data, first.ctypes.data, None if stats is None else C.addressof(stats),
                              None, None, None, None, None, 0, 0)
        totals = N.gx_lookup_totals()
        nl = C.c_uint64(0)
        _check(N.lib().gx_text_lookup_lines(self._h.ptr, raw.ctypes.data if raw.size else None, raw.size, parts.array, parts.n, terms.array, terms.n,
                                            eu.ctypes.data if eu.size else None, eo.ctypes.data if m else None, m, keep, N.GX_GROUP_WEAK_HASH if weak_hash else 0,
                                            C.byref(out), data.ctypes.data if keep else None, raw.size, koff.ctypes.data if keep else None,
                                            index.ctypes.data if keep else None, C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o)))
        totals = self._lookup_totals(totals)
        res = self._lookup_result(parts, m, line_entry[:nl.value], same, lines, first, stats, totals)
        if keep:
            k = totals["lines_out"]
            res.update(index=index[:k], data=data[:totals["units_out"]], offsets=koff[:k + 1])
        return res, counts, nl.value

    # -- lines grouped by two captured texts (gx_group_pairs / gx_text_group_pairs) ----------------------------------------------
    def pair_parts(self, spec):
        """Resolves a list of (extraction, key extractor, second extractor[, value extractor]) into (GroupParts, int32 second groups):
        the first, second and optional fourth entry as group_parts takes a part, the third the extractor whose value is the line's
        SECOND (None: the part's lines have a key and no second).  A (GroupParts, seconds) tuple passes through."""
        if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], GroupParts):
            return spec
        spec = [tuple(item) for item in spec]
        for item in spec:
            if len(item) not in (3, 4):
                raise ValueError("a part is (extraction, key extractor, second extractor[, value extractor])")
        parts = self.group_parts([(item[0], item[1]) + tuple(item[3:]) for item in spec])
        seconds = (C.c_int32 * max(1, len(spec)))()
        for t, item in enumerate(spec):
            seconds[t] = -1 if item[2] is None else self._extraction_and_group(parts.array[t].extraction, item[2])[1]
        return parts, seconds

    @staticmethod
    def _pairs_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(n_pairs=t.n_pairs, pair_units=t.pair_units, paired=t.paired, unpaired=t.unpaired, pairs_exact=bool(t.pairs_exact))
        return d

    def group_pairs_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                           key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, pair_units_ptr=None, pair_units_cap=0,
                           pair_offsets_ptr=None, pair_key_ptr=None, pair_first_line_ptr=None, pair_lines_ptr=None, key_pairs_ptr=None, line_pair_ptr=None,
                           max_pairs=0, pairs=True, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_group_pairs on device pointers (ints): group_lines_device's keys, plus the pairs (key, second text) in the caller's
        buffers, each optional (none at all: the size query; max_keys and max_pairs still size the tables).  pairs=False passes
        pairs == NULL: the call is gx_group_lines.  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and
        totals says what the outputs need (n_keys, key_units, n_pairs, pair_units; exact / pairs_exact False: that table overflowed,
        the number of lines always suffices); every other error raises."""
        parts, seconds = self.pair_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_pairs_out(pair_units_ptr, pair_units_cap, pair_offsets_ptr, pair_key_ptr, pair_first_line_ptr, pair_lines_ptr, key_pairs_ptr, line_pair_ptr, max_pairs)
        totals = N.gx_pairs_totals()
        rc = N.lib().gx_group_pairs(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, seconds, terms.array, terms.n,
                                    N.GX_GROUP_WEAK_HASH if weak_hash else 0, C.byref(keys), C.byref(out) if pairs else None, C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._pairs_totals(totals)

    def text_group_pairs_device(self, text_ptr, size, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None, key_first_line_ptr=None,
                                key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, pair_units_ptr=None, pair_units_cap=0, pair_offsets_ptr=None,
                                pair_key_ptr=None, pair_first_line_ptr=None, pair_lines_ptr=None, key_pairs_ptr=None, line_pair_ptr=None, max_pairs=0, pairs=True,
                                offsets64=False, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_text_group_pairs on a device buffer (int); outputs as group_pairs_device takes them (line_key and line_pair: one entry per
        line of the text).  Returns (rc, totals, counts, n_lines)."""
        parts, seconds = self.pair_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_pairs_out(pair_units_ptr, pair_units_cap, pair_offsets_ptr, pair_key_ptr, pair_first_line_ptr, pair_lines_ptr, key_pairs_ptr, line_pair_ptr, max_pairs)
        totals = N.gx_pairs_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_pairs(self._h.ptr, text_ptr, size, parts.array, parts.n, seconds, terms.array, terms.n, N.GX_GROUP_WEAK_HASH if weak_hash else 0,
                                         C.byref(keys), C.byref(out) if pairs else None, C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._pairs_totals(totals), counts, nl.value

    def _pairs_host(self, device_call, n_lines_cap, units_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap, max_pairs, pair_units_cap):
        """_group_host with the pair arrays beside the key arrays.  max_pairs defaults to the number of lines and pair_units_cap to the
        batch's units, which always suffice (no more pairs than lines, and a pair's second is a part of its first line); smaller ones
        are raised to what a GX_E_LIMIT reports."""
        size = {"max_pairs": n_lines_cap if max_pairs is None else max_pairs, "pair_units_cap": units_cap if pair_units_cap is None else pair_units_cap}
        got = {}

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            mp, pc = size["max_pairs"], size["pair_units_cap"]
            got.update(pair_units=np.zeros(max(1, pc), unit_dtype), pair_offsets=np.zeros(mp + 1, offsets_dtype), pair_key=np.zeros(max(1, mp), np.uint32),
                       pair_first_line=np.zeros(max(1, mp), np.uint32), pair_lines=np.zeros(max(1, mp), np.uint64), key_pairs=np.zeros(max(1, mk), np.uint64),
                       line_pair=np.full(max(1, n_lines_cap), 0xFFFFFFFF, np.uint32))
            r = device_call(units, cap, koff, first, lines, stats, line_key, mk, got["pair_units"].ctypes.data, pc, got["pair_offsets"].ctypes.data,
                            got["pair_key"].ctypes.data, got["pair_first_line"].ctypes.data, got["pair_lines"].ctypes.data, got["key_pairs"].ctypes.data,
                            got["line_pair"].ctypes.data, mp)
            if r[0] == N.GX_E_LIMIT and r[1]["exact"]:
                if r[1]["pairs_exact"]:
                    size.update(max_pairs=max(mp, r[1]["n_pairs"]), pair_units_cap=max(pc, r[1]["pair_units"]))
                else:
                    size["max_pairs"] = n_lines_cap
            return r
        res, rest = self._group_host(call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap)
        p, k = res["totals"]["n_pairs"], res["totals"]["n_keys"]
        poff, punits = got["pair_offsets"][:p + 1], got["pair_units"][:res["totals"]["pair_units"]]
        res.update(pair_units=punits, pair_offsets=poff, pair_key=got["pair_key"][:p], pair_first_line=got["pair_first_line"][:p], pair_lines=got["pair_lines"][:p],
                   key_pairs=got["key_pairs"][:k], line_pair=got["line_pair"])
        if keys == "list":
            res["pairs"] = [(int(got["pair_key"][j]), decode(punits[int(poff[j]):int(poff[j + 1])])) for j in range(p)]
        return res, rest

    def group_pairs(self, data, offsets, ids, rows, parts, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None, max_pairs=None,
                    pair_units_cap=None, weak_hash=False):
        """gx_group_pairs on host buffers: group_lines' keys, and the lines grouped by (key, second text) -- GROUP BY a, b and
        COUNT(DISTINCT b) GROUP BY a.  parts: (extraction, key extractor, second extractor[, value extractor]) each (pair_parts);
        everything else as group_lines takes it.  Returns group_lines' dict plus pairs (a list of (key number, second) in order of
        first appearance; keys="csr": pair_units / pair_offsets / pair_key alone, which are always there), pair_lines, pair_first_line
        (per pair), key_pairs (per key: its distinct seconds), line_pair (uint32 per input line, 0xFFFFFFFF: none) and the pair totals
        (n_pairs, pair_units, paired, unpaired, pairs_exact) in totals.  max_pairs defaults to the number of lines."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        both = self.pair_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.group_pairs_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), both, where, *outs, offsets64=offsets.dtype == np.uint64,
                                           utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8), weak_hash=weak_hash)
        res, _ = self._pairs_host(device_call, n, int(offsets[n] - offsets[0]) if n else 0, both[0], data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap,
                                  max_pairs, pair_units_cap)
        res["line_key"], res["line_pair"] = res["line_key"][:n], res["line_pair"][:n]
        return res

    def text_group_pairs(self, text, parts, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None, max_pairs=None, pair_units_cap=None):
        """gx_text_group_pairs on a host buffer: raw text -> lines -> extraction -> group_pairs.  Returns (the dict group_pairs returns,
        counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        both = self.pair_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.text_group_pairs_device(raw.ctypes.data if raw.size else None, raw.size, both, where, *outs, device_pointers=False, utf8=utf8)
        res, (counts, n_lines) = self._pairs_host(device_call, cap_lines, raw.size, both[0], np.uint8, np.uint32, keys, decode, max_keys, key_units_cap, max_pairs,
                                                  pair_units_cap)
        res["line_key"], res["line_pair"] = res["line_key"][:n_lines], res["line_pair"][:n_lines]
        return res, counts, n_lines

    # -- lines per interval of a captured number (gx_bucket_lines / gx_text_bucket_lines) ------------------------------------------
    def bucket_parts(self, spec):
        """Resolves a list of (extraction, number extractor) or (extraction, number extractor, value extractor) into gx_bucket_part
        records, names and indices as group_parts takes them: ("Syslog", "ts") or ("GetRequest", "ts", "timeTakenInMsec").  At most
        one part per extraction, at most 64 parts.  Returns a BucketParts; a BucketParts passes through."""
        if isinstance(spec, BucketParts):
            return spec
        spec = list(spec)
        if len(spec) > 64:
            raise ValueError("at most 64 parts")
        arr = (N.gx_bucket_part * max(1, len(spec)))()
        seen = set()
        for t, item in enumerate(spec):
            item = tuple(item)
            if len(item) == 2:
                item = item + (None,)
            if len(item) != 3:
                raise ValueError("a part is (extraction, number extractor[, value extractor])")
            k, g = self._extraction_and_group(item[0], item[1])
            if k in seen:
                raise ValueError("two parts for extraction %r" % (item[0],))
            seen.add(k)
            arr[t].extraction, arr[t].number_group, arr[t].value_group = k, g, -1 if item[2] is None else self._extraction_and_group(k, item[2])[1]
        return BucketParts(arr, len(spec))

    def _bucket_origin(self, parts, origin):
        """origin as an int; a str or bytes is read with parse_number under the first part's number format."""
        if isinstance(origin, (str, bytes, bytearray)):
            if not parts.n:
                raise ValueError("a text origin needs a part: it is read under the first part's number format")
            kind, scale = self.number_format(parts.array[0].extraction, parts.array[0].number_group)
            value = parse_number(kind, scale, origin)
            if value is None:
                raise ValueError("origin %r is no number under the format (%s, %d)" % (origin, kind, scale))
            return value
        if isinstance(origin, bool) or not isinstance(origin, (int, np.integer)) or not -2 ** 63 <= int(origin) < 2 ** 63:
            raise ValueError("origin: an int64, or a text read under the first part's number format")
        return int(origin)

    @staticmethod
    def _bucket_totals(t):
        return {"n_buckets": t.n_buckets, "lines": t.lines, "bucketed": t.bucketed, "unset": t.unset, "not_numbers": t.not_numbers,
                "out_of_range": t.out_of_range, "exact": bool(t.exact), "first_bucket": t.first_bucket, "last_bucket": t.last_bucket}

    @staticmethod
    def _bucket_flags(weak_hash, all_digits):
        return (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (N.GX_BUCKET_ALL_DIGITS if all_digits else 0)

    def bucket_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, width, origin=0, where=None, bucket_number_ptr=None,
                            bucket_first_line_ptr=None, bucket_lines_ptr=None, bucket_stats_ptr=None, line_bucket_ptr=None, max_buckets=0, offsets64=False,
                            utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_bucket_lines on device pointers (ints); the outputs are the caller's buffers, each optional (none at all: the size query;
        max_buckets still sizes the table).  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals
        says what the outputs need (n_buckets; exact False: the table overflowed, max_buckets = n always suffices); every other error
        raises."""
        parts = self.bucket_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_bucket_out(bucket_number_ptr, bucket_first_line_ptr, bucket_lines_ptr, bucket_stats_ptr, line_bucket_ptr, max_buckets)
        totals = N.gx_bucket_totals()
        rc = N.lib().gx_bucket_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, self._bucket_origin(parts, origin), int(width),
                                     terms.array, terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(out), C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_buckets):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._bucket_totals(totals)

    def text_bucket_lines_device(self, text_ptr, size, parts, width, origin=0, where=None, bucket_number_ptr=None, bucket_first_line_ptr=None,
                                 bucket_lines_ptr=None, bucket_stats_ptr=None, line_bucket_ptr=None, max_buckets=0, stream=None, device_pointers=True, utf8=False,
                                 weak_hash=False, all_digits=False):
        """gx_text_bucket_lines on a device buffer (int); outputs as bucket_lines_device takes them (line_bucket: one entry per line of
        the text).  Returns (rc, totals, counts, n_lines)."""
        parts = self.bucket_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out = N.gx_bucket_out(bucket_number_ptr, bucket_first_line_ptr, bucket_lines_ptr, bucket_stats_ptr, line_bucket_ptr, max_buckets)
        totals = N.gx_bucket_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_bucket_lines(self._h.ptr, text_ptr, size, parts.array, parts.n, self._bucket_origin(parts, origin), int(width), terms.array, terms.n,
                                          self._bucket_flags(weak_hash, all_digits), C.byref(out), C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_buckets):
            _check(rc)
        return rc, self._bucket_totals(totals), counts, nl.value

    def _bucket_host(self, call, n_lines_cap, parts, max_buckets):
        """Runs `call(out arrays..., max_buckets)` on host arrays; on GX_E_LIMIT once more with the size it reported when it is exact,
        else with the number of lines (which may report an exact size in turn): three calls at the most.  Builds the result dict."""
        max_buckets = min(n_lines_cap, 1024) if max_buckets is None else max_buckets
        for attempt in range(3):
            number = np.zeros(max(1, max_buckets), np.int64)
            first = np.zeros(max(1, max_buckets), np.uint32)
            lines = np.zeros(max(1, max_buckets), np.uint64)
            stats = (N.gx_measure_stats * max(1, max_buckets))() if parts.has_values else None
            line_bucket = np.full(max(1, n_lines_cap), 0xFFFFFFFF, np.uint32)
            got = call(number.ctypes.data, first.ctypes.data, lines.ctypes.data, None if stats is None else C.addressof(stats), line_bucket.ctypes.data, max_buckets)
            rc, totals = got[0], got[1]
            if rc == N.GX_OK:
                break
            if attempt == 2:
                raise GorpError(rc, N.last_error())
            max_buckets = max(max_buckets, totals["n_buckets"]) if totals["exact"] else n_lines_cap
        k = totals["n_buckets"]
        res = {"bucket_number": number[:k], "first_line": first[:k], "lines": lines[:k], "totals": totals, "line_bucket": line_bucket,
               "stats": None if stats is None else [{"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                                                      "min": s.min if s.numbers else None, "max": s.max if s.numbers else None,
                                                      "sum": (s.sum_hi << 64) + s.sum_lo} for s in stats[:k]]}
        return res, got[2:]

    def bucket_lines(self, data, offsets, match_id, caps, parts, width, origin=0, where=None, max_buckets=None, utf8=None, weak_hash=False, all_digits=False):
        """gx_bucket_lines on host buffers: the lines counted -- and, with a value extractor, measured -- per interval
        floor((number - origin) / width) of the number the part of their extraction names (parts: Gorp.bucket_parts or its input), of
        the lines on which every term of `where` holds.  The number is read under its group's number format (set_number_format), so
        with ("Syslog", "ts") read as iso8601 at scale 3 and width 60_000 the buckets are minutes; origin is an int in the format's
        unit, or a text read under the first part's format.  data / offsets / match_id / caps and utf8 as group_lines takes them.
        Returns a dict: bucket_number (int64, ascending; only occupied buckets), first_line, lines (per bucket), stats (per bucket, as
        group_lines gives them per key; None when no part has a value extractor), line_bucket (uint32 per input line: the index of its
        bucket in bucket_number, 0xFFFFFFFF: none) and totals."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(match_id)
        compact = self._ids_format(ids)
        rows = None if caps is None or compact else np.ascontiguousarray(caps, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.bucket_parts(parts)
        n = len(offsets) - 1

        def call(number, first, lines, stats, line_bucket, mb):
            return self.bucket_lines_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(rows), parts, width, origin, where, number, first, lines, stats,
                                            line_bucket, mb, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False,
                                            utf8=bool(utf8), weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._bucket_host(call, n, parts, max_buckets)
        res["line_bucket"] = res["line_bucket"][:n]
        return res

    def text_bucket_lines(self, text, parts, width, origin=0, where=None, max_buckets=None, utf8=False, weak_hash=False, all_digits=False):
        """gx_text_bucket_lines on a host buffer: raw text -> lines -> extraction -> bucket_lines.  Returns (the dict bucket_lines
        returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.bucket_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)

        def call(number, first, lines, stats, line_bucket, mb):
            return self.text_bucket_lines_device(raw.ctypes.data if raw.size else None, raw.size, parts, width, origin, where, number, first, lines, stats, line_bucket,
                                                 mb, device_pointers=False, utf8=utf8, weak_hash=weak_hash, all_digits=all_digits)
        res, (counts, n_lines) = self._bucket_host(call, cap_lines, parts, max_buckets)
        res["line_bucket"] = res["line_bucket"][:n_lines]
        return res, counts, n_lines

    # -- a series per captured text: lines per (key, interval of a captured number) (gx_group_series / gx_text_group_series) ---------
    def series_parts(self, spec):
        """Resolves a list of (extraction, key extractor, number extractor[, value extractor]) into (GroupParts, int32 number groups):
        the first, second and optional fourth entry as group_parts takes a part, the third the extractor whose value is the line's
        NUMBER (None: the part's lines have a key and no number, -1).  A (GroupParts, numbers) tuple passes through."""
        if isinstance(spec, tuple) and len(spec) == 2 and isinstance(spec[0], GroupParts):
            return spec
        spec = [tuple(item) for item in spec]
        for item in spec:
            if len(item) not in (3, 4):
                raise ValueError("a part is (extraction, key extractor, number extractor[, value extractor])")
        parts = self.group_parts([(item[0], item[1]) + tuple(item[3:]) for item in spec])
        numbers = (C.c_int32 * max(1, len(spec)))()
        for t, item in enumerate(spec):
            numbers[t] = -1 if item[2] is None else self._extraction_and_group(parts.array[t].extraction, item[2])[1]
        return parts, numbers

    def _series_origin(self, both, origin):
        """origin as an int; a text is read by _bucket_origin's rule under the number format of the first part that has a number."""
        parts, numbers = both
        numbered = [(parts.array[t].extraction, numbers[t]) for t in range(parts.n) if numbers[t] >= 0]
        return self._bucket_origin(self.bucket_parts(numbered[:1]), origin)

    @staticmethod
    def _series_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(n_cells=t.n_cells, n_buckets=t.n_buckets, celled=t.celled, number_unset=t.number_unset, not_numbers=t.not_numbers,
                 out_of_range=t.out_of_range, cells_exact=bool(t.cells_exact), first_bucket=t.first_bucket, last_bucket=t.last_bucket,
                 group=Gorp._group_totals(t.group))
        return d

    def group_series_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, width, origin=0, where=None, key_units_ptr=None, key_units_cap=0,
                            key_offsets_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0,
                            bucket_number_ptr=None, cell_key_ptr=None, cell_bucket_ptr=None, cell_first_line_ptr=None, cell_lines_ptr=None, cell_stats_ptr=None,
                            key_cell_begin_ptr=None, line_cell_ptr=None, max_cells=0, max_buckets=0, series=True, offsets64=False, utf16=False, compact=0,
                            stream=None, device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_group_series on device pointers (ints): group_lines_device's keys, plus the cells (key, bucket) in the caller's buffers,
        each optional (none at all: the size query; max_keys and max_cells still size the tables).  series=False passes series ==
        NULL: the call is gx_group_lines.  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says
        what the outputs need (n_keys, key_units, n_cells, n_buckets; exact / cells_exact False: that table overflowed, the number of
        lines always suffices); every other error raises."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_series_out(bucket_number_ptr, cell_key_ptr, cell_bucket_ptr, cell_first_line_ptr, cell_lines_ptr, cell_stats_ptr, key_cell_begin_ptr, line_cell_ptr,
                              max_cells, max_buckets)
        totals = N.gx_series_totals()
        rc = N.lib().gx_group_series(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, both[0].array, both[0].n, both[1], self._series_origin(both, origin),
                                     int(width), terms.array, terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(keys), C.byref(out) if series else None,
                                     C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._series_totals(totals)

    def text_group_series_device(self, text_ptr, size, parts, width, origin=0, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                                 key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, bucket_number_ptr=None,
                                 cell_key_ptr=None, cell_bucket_ptr=None, cell_first_line_ptr=None, cell_lines_ptr=None, cell_stats_ptr=None, key_cell_begin_ptr=None,
                                 line_cell_ptr=None, max_cells=0, max_buckets=0, series=True, offsets64=False, stream=None, device_pointers=True, utf8=False,
                                 weak_hash=False, all_digits=False):
        """gx_text_group_series on a device buffer (int); outputs as group_series_device takes them (line_key and line_cell: one entry
        per line of the text).  Returns (rc, totals, counts, n_lines)."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_series_out(bucket_number_ptr, cell_key_ptr, cell_bucket_ptr, cell_first_line_ptr, cell_lines_ptr, cell_stats_ptr, key_cell_begin_ptr, line_cell_ptr,
                              max_cells, max_buckets)
        totals = N.gx_series_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_series(self._h.ptr, text_ptr, size, both[0].array, both[0].n, both[1], self._series_origin(both, origin), int(width), terms.array,
                                          terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(keys), C.byref(out) if series else None, C.byref(totals),
                                          counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._series_totals(totals), counts, nl.value

    def _series_host(self, device_call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap, max_cells, max_buckets):
        """_group_host with the series arrays beside the key arrays.  max_cells defaults to min(the number of lines, 4 096) and
        max_buckets to max_cells; an exact GX_E_LIMIT raises them to what it reports, an overflowed key or cell table to the number
        of lines, which always suffices: behind any overflow the next call's tables hold everything, so three calls are enough."""
        mc0 = min(n_lines_cap, 4096) if max_cells is None else max_cells
        size = {"max_cells": mc0, "max_buckets": mc0 if max_buckets is None else max_buckets}
        got = {}

        def call(units, cap, koff, first, lines, stats, line_key, mk):
            mc, mb = size["max_cells"], size["max_buckets"]
            got.update(bucket_number=np.zeros(max(1, mb), np.int64), cell_key=np.zeros(max(1, mc), np.uint32), cell_bucket=np.zeros(max(1, mc), np.uint32),
                       cell_first_line=np.zeros(max(1, mc), np.uint32), cell_lines=np.zeros(max(1, mc), np.uint64),
                       cell_stats=(N.gx_measure_stats * max(1, mc))() if parts.has_values else None, key_cell_begin=np.zeros(mk + 1, np.uint64),
                       line_cell=np.full(max(1, n_lines_cap), 0xFFFFFFFF, np.uint32))
            r = device_call(units, cap, koff, first, lines, stats, line_key, mk, got["bucket_number"].ctypes.data, got["cell_key"].ctypes.data,
                            got["cell_bucket"].ctypes.data, got["cell_first_line"].ctypes.data, got["cell_lines"].ctypes.data,
                            None if got["cell_stats"] is None else C.addressof(got["cell_stats"]), got["key_cell_begin"].ctypes.data, got["line_cell"].ctypes.data, mc, mb)
            if r[0] == N.GX_E_LIMIT and r[1]["exact"] and r[1]["cells_exact"]:
                size.update(max_cells=max(mc, r[1]["n_cells"]), max_buckets=max(mb, r[1]["n_buckets"]))
            elif r[0] == N.GX_E_LIMIT:
                # A table overflowed.  The key table's overflow leaves the series totals zero, so nothing is known of the cells: both
                # series sizes go to the number of lines with it, and the limits of keys and cells never take a call each.
                size.update(max_cells=n_lines_cap, max_buckets=max(mb, n_lines_cap) if max_buckets is None else mb)
            return r
        res, rest = self._group_host(call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap)
        c, b, k = res["totals"]["n_cells"], res["totals"]["n_buckets"], res["totals"]["n_keys"]
        st = got["cell_stats"]
        res.update(bucket_number=got["bucket_number"][:b], cell_key=got["cell_key"][:c], cell_bucket=got["cell_bucket"][:c], cell_first_line=got["cell_first_line"][:c],
                   cell_lines=got["cell_lines"][:c], key_cell_begin=got["key_cell_begin"][:k + 1], line_cell=got["line_cell"],
                   cell_stats=None if st is None else [{"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                                                        "min": s.min if s.numbers else None, "max": s.max if s.numbers else None,
                                                        "sum": (s.sum_hi << 64) + s.sum_lo} for s in st[:c]])
        return res, rest

    def group_series(self, data, offsets, ids, rows, parts, width, origin=0, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None, max_cells=None,
                     max_buckets=None, weak_hash=False, all_digits=False):
        """gx_group_series on host buffers: group_lines' keys, and the lines counted -- and, with a value extractor, measured -- per
        (key, interval floor((number - origin) / width)): GROUP BY verb, minute.  parts: (extraction, key extractor, number
        extractor[, value extractor]) each (series_parts); width and origin as bucket_lines takes them (a text origin is read under
        the first numbered part's number format); everything else as group_lines takes it.  Returns group_lines' dict plus
        bucket_number (the axis: int64, ascending, the buckets that hold a cell), cell_key, cell_bucket (the index into
        bucket_number), cell_first_line, cell_lines, cell_stats (per cell, ordered by (key number, bucket); None when no part has a
        value extractor), key_cell_begin (n_keys + 1: key j's cells are [begin[j], begin[j + 1])), line_cell (uint32 per input line,
        0xFFFFFFFF: none) and the series totals (n_cells, n_buckets, celled, number_unset, not_numbers, out_of_range, cells_exact,
        first_bucket, last_bucket) in totals.  On an exact GX_E_LIMIT the call is repeated once with the sizes it reported."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        both = self.series_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.group_series_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), both, width, origin, where, *outs,
                                            offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8),
                                            weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._series_host(device_call, n, both[0], data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap, max_cells, max_buckets)
        res["line_key"], res["line_cell"] = res["line_key"][:n], res["line_cell"][:n]
        return res

    def text_group_series(self, text, parts, width, origin=0, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None, max_cells=None,
                          max_buckets=None, weak_hash=False, all_digits=False):
        """gx_text_group_series on a host buffer: raw text -> lines -> extraction -> group_series.  Returns (the dict group_series
        returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        both = self.series_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.text_group_series_device(raw.ctypes.data if raw.size else None, raw.size, both, width, origin, where, *outs, device_pointers=False, utf8=utf8,
                                                 weak_hash=weak_hash, all_digits=all_digits)
        res, (counts, n_lines) = self._series_host(device_call, cap_lines, both[0], np.uint8, np.uint32, keys, decode, max_keys, key_units_cap, max_cells, max_buckets)
        res["line_key"], res["line_cell"] = res["line_key"][:n_lines], res["line_cell"][:n_lines]
        return res, counts, n_lines

    # -- sessions per captured text: a key's lines in time order, cut at gaps (gx_group_sessions / gx_text_group_sessions) ----------
    def _sessions_gap(self, both, max_gap):
        """max_gap as an int >= 0; a text is read as _series_origin reads an origin, under the first numbered part's number format."""
        try:
            gap = self._series_origin(both, max_gap)
        except ValueError:
            gap = -1
        if gap < 0:
            raise ValueError("max_gap %r: an int64 >= 0, or a text read under the first timed part's number format" % (max_gap,))
        return gap

    @staticmethod
    def _sessions_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(n_sessions=t.n_sessions, entries=t.entries, number_unset=t.number_unset, not_numbers=t.not_numbers, longest_lines=t.longest_lines,
                 longest_duration=t.longest_duration, first_time=t.first_time, last_time=t.last_time, group=Gorp._group_totals(t.group))
        return d

    def group_sessions_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, max_gap, where=None, key_units_ptr=None, key_units_cap=0,
                              key_offsets_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0,
                              session_key_ptr=None, session_begin_ptr=None, session_end_ptr=None, session_first_line_ptr=None, session_lines_ptr=None,
                              session_stats_ptr=None, session_entry_begin_ptr=None, key_session_begin_ptr=None, entry_line_ptr=None, line_session_ptr=None,
                              max_sessions=0, max_entries=0, sessions=True, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True,
                              utf8=False, weak_hash=False, all_digits=False):
        """gx_group_sessions on device pointers (ints): group_lines_device's keys, plus the sessions in the caller's buffers, each
        optional (none at all: the size query; max_keys still sizes the table).  parts as series_parts takes them: the number is the
        line's TIME.  sessions=False passes sessions == NULL: the call is gx_group_lines.  Returns (rc, totals): rc is GX_OK or
        GX_E_LIMIT -- then nothing was written and totals says what the outputs need (n_keys, key_units, n_sessions, entries; entries
        always suffices for max_sessions and max_entries); every other error raises."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_sessions_out(session_key_ptr, session_begin_ptr, session_end_ptr, session_first_line_ptr, session_lines_ptr, session_stats_ptr,
                                session_entry_begin_ptr, key_session_begin_ptr, entry_line_ptr, line_session_ptr, max_sessions, max_entries)
        totals = N.gx_sessions_totals()
        rc = N.lib().gx_group_sessions(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, both[0].array, both[0].n, both[1], self._sessions_gap(both, max_gap),
                                       terms.array, terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(keys), C.byref(out) if sessions else None,
                                       C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._sessions_totals(totals)

    def text_group_sessions_device(self, text_ptr, size, parts, max_gap, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                                   key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, session_key_ptr=None,
                                   session_begin_ptr=None, session_end_ptr=None, session_first_line_ptr=None, session_lines_ptr=None, session_stats_ptr=None,
                                   session_entry_begin_ptr=None, key_session_begin_ptr=None, entry_line_ptr=None, line_session_ptr=None, max_sessions=0,
                                   max_entries=0, sessions=True, offsets64=False, stream=None, device_pointers=True, utf8=False, weak_hash=False,
                                   all_digits=False):
        """gx_text_group_sessions on a device buffer (int); outputs as group_sessions_device takes them (line_key and line_session: one
        entry per line of the text).  Returns (rc, totals, counts, n_lines)."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_sessions_out(session_key_ptr, session_begin_ptr, session_end_ptr, session_first_line_ptr, session_lines_ptr, session_stats_ptr,
                                session_entry_begin_ptr, key_session_begin_ptr, entry_line_ptr, line_session_ptr, max_sessions, max_entries)
        totals = N.gx_sessions_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_sessions(self._h.ptr, text_ptr, size, both[0].array, both[0].n, both[1], self._sessions_gap(both, max_gap), terms.array, terms.n,
                                            self._bucket_flags(weak_hash, all_digits), C.byref(keys), C.byref(out) if sessions else None, C.byref(totals),
                                            counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._sessions_totals(totals), counts, nl.value

    def _sessions_host(self, device_call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap):
        """_group_host with the session arrays beside the key arrays, each sized by the number of lines: no more entries than lines, no
        more sessions than entries."""
        got = {}
        cap = max(1, n_lines_cap)

        def call(units, ucap, koff, first, lines, stats, line_key, mk):
            got.update(session_key=np.zeros(cap, np.uint32), session_begin=np.zeros(cap, np.int64), session_end=np.zeros(cap, np.int64),
                       session_first_line=np.zeros(cap, np.uint32), session_lines=np.zeros(cap, np.uint64),
                       session_stats=(N.gx_measure_stats * cap)() if parts.has_values else None, session_entry_begin=np.zeros(cap + 1, np.uint64),
                       key_session_begin=np.zeros(mk + 1, np.uint64), entry_line=np.zeros(cap, np.uint32), line_session=np.full(cap, 0xFFFFFFFF, np.uint32))
            return device_call(units, ucap, koff, first, lines, stats, line_key, mk, got["session_key"].ctypes.data, got["session_begin"].ctypes.data,
                               got["session_end"].ctypes.data, got["session_first_line"].ctypes.data, got["session_lines"].ctypes.data,
                               None if got["session_stats"] is None else C.addressof(got["session_stats"]), got["session_entry_begin"].ctypes.data,
                               got["key_session_begin"].ctypes.data, got["entry_line"].ctypes.data, got["line_session"].ctypes.data, n_lines_cap, n_lines_cap)
        res, rest = self._group_host(call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap)
        s, m, k = res["totals"]["n_sessions"], res["totals"]["entries"], res["totals"]["n_keys"]
        st = got["session_stats"]
        res.update(session_key=got["session_key"][:s], session_begin=got["session_begin"][:s], session_end=got["session_end"][:s],
                   session_first_line=got["session_first_line"][:s], session_lines=got["session_lines"][:s], session_entry_begin=got["session_entry_begin"][:s + 1],
                   key_session_begin=got["key_session_begin"][:k + 1], entry_line=got["entry_line"][:m], line_session=got["line_session"],
                   session_stats=None if st is None else [{"lines": x.lines, "numbers": x.numbers, "unset": x.unset, "not_numbers": x.not_numbers,
                                                           "min": x.min if x.numbers else None, "max": x.max if x.numbers else None,
                                                           "sum": (x.sum_hi << 64) + x.sum_lo} for x in st[:s]])
        return res, rest

    def group_sessions(self, data, offsets, ids, rows, parts, max_gap, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None, weak_hash=False,
                       all_digits=False):
        """gx_group_sessions on host buffers: group_lines' keys, and every key's lines ordered by a captured time and cut into SESSIONS: a
        new one at the key's first entry and wherever the time exceeds the previous entry's by more than max_gap -- Splunk's
        `transaction id maxpause=`.  parts: (extraction, key extractor, time extractor[, value extractor]) each (series_parts); max_gap
        an int >= 0 in the time's own unit, or a text read under the first timed part's number format; everything else as group_lines
        takes it.  Returns group_lines' dict plus session_key, session_begin, session_end, session_first_line, session_lines,
        session_stats (per session, ordered by (key number, begin); None when no part has a value extractor), session_entry_begin
        (n_sessions + 1: session s's entries are entry_line[begin[s]:begin[s + 1]]), key_session_begin (n_keys + 1), entry_line (the
        entries' input lines ordered by (key, time, line)), line_session (uint32 per input line, 0xFFFFFFFF: no entry) and the session
        totals (n_sessions, entries, number_unset, not_numbers, longest_lines, longest_duration, first_time, last_time) in totals."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        both = self.series_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.group_sessions_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), both, max_gap, where, *outs,
                                              offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8),
                                              weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._sessions_host(device_call, n, both[0], data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap)
        res["line_key"], res["line_session"] = res["line_key"][:n], res["line_session"][:n]
        return res

    def text_group_sessions(self, text, parts, max_gap, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None, weak_hash=False, all_digits=False):
        """gx_text_group_sessions on a host buffer: raw text -> lines -> extraction -> group_sessions.  Returns (the dict group_sessions
        returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        both = self.series_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.text_group_sessions_device(raw.ctypes.data if raw.size else None, raw.size, both, max_gap, where, *outs, device_pointers=False, utf8=utf8,
                                                   weak_hash=weak_hash, all_digits=all_digits)
        res, (counts, n_lines) = self._sessions_host(device_call, cap_lines, both[0], np.uint8, np.uint32, keys, decode, max_keys, key_units_cap)
        res["line_key"], res["line_session"] = res["line_key"][:n_lines], res["line_session"][:n_lines]
        return res, counts, n_lines

    # -- trailing time windows per captured text: a key's lines within the last W before each (gx_group_windows / gx_text_group_windows) --
    WINDOW_OUTS = ("entry_line", "entry_key", "entry_time", "entry_window_lines", "entry_window_sum", "key_entry_begin", "key_peak_lines", "key_peak_line",
                   "line_window_lines", "trip_key", "trip_line", "trip_time", "trip_entry", "key_trip_begin")

    def _windows_window(self, both, window):
        """window as an int >= 0, taken as group_sessions takes max_gap."""
        try:
            return self._sessions_gap(both, window)
        except ValueError:
            raise ValueError("window %r: an int64 >= 0, or a text read under the first timed part's number format" % (window,)) from None

    @staticmethod
    def _windows_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(entries=t.entries, number_unset=t.number_unset, not_numbers=t.not_numbers, n_trips=t.n_trips, tripped_keys=t.tripped_keys,
                 peak_lines=t.peak_lines, peak_line=t.peak_line, peak_key=t.peak_key, first_time=t.first_time, last_time=t.last_time,
                 group=Gorp._group_totals(t.group))
        return d

    def group_windows_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, window, threshold=0, where=None, key_units_ptr=None, key_units_cap=0,
                             key_offsets_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0,
                             entry_line_ptr=None, entry_key_ptr=None, entry_time_ptr=None, entry_window_lines_ptr=None, entry_window_sum_ptr=None,
                             key_entry_begin_ptr=None, key_peak_lines_ptr=None, key_peak_line_ptr=None, line_window_lines_ptr=None, trip_key_ptr=None,
                             trip_line_ptr=None, trip_time_ptr=None, trip_entry_ptr=None, key_trip_begin_ptr=None, max_entries=0, max_trips=0, windows=True,
                             offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_group_windows on device pointers (ints): group_lines_device's keys, plus the windows in the caller's buffers, each optional
        (none at all: the size query; max_keys still sizes the table).  parts as series_parts takes them: the number is the line's
        TIME.  windows=False passes windows == NULL: the call is gx_group_lines.  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT --
        then nothing was written and totals says what the outputs need (n_keys, key_units, entries, n_trips; entries always suffices
        for max_entries and max_trips); every other error raises."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_windows_out(entry_line_ptr, entry_key_ptr, entry_time_ptr, entry_window_lines_ptr, entry_window_sum_ptr, key_entry_begin_ptr, key_peak_lines_ptr,
                               key_peak_line_ptr, line_window_lines_ptr, trip_key_ptr, trip_line_ptr, trip_time_ptr, trip_entry_ptr, key_trip_begin_ptr, max_entries,
                               max_trips)
        totals = N.gx_windows_totals()
        rc = N.lib().gx_group_windows(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, both[0].array, both[0].n, both[1], self._windows_window(both, window),
                                      int(threshold), terms.array, terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(keys),
                                      C.byref(out) if windows else None, C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._windows_totals(totals)

    def text_group_windows_device(self, text_ptr, size, parts, window, threshold=0, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                                  key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, entry_line_ptr=None,
                                  entry_key_ptr=None, entry_time_ptr=None, entry_window_lines_ptr=None, entry_window_sum_ptr=None, key_entry_begin_ptr=None,
                                  key_peak_lines_ptr=None, key_peak_line_ptr=None, line_window_lines_ptr=None, trip_key_ptr=None, trip_line_ptr=None,
                                  trip_time_ptr=None, trip_entry_ptr=None, key_trip_begin_ptr=None, max_entries=0, max_trips=0, windows=True, offsets64=False,
                                  stream=None, device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_text_group_windows on a device buffer (int); outputs as group_windows_device takes them (line_key and line_window_lines: one
        entry per line of the text).  Returns (rc, totals, counts, n_lines)."""
        both = self.series_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_windows_out(entry_line_ptr, entry_key_ptr, entry_time_ptr, entry_window_lines_ptr, entry_window_sum_ptr, key_entry_begin_ptr, key_peak_lines_ptr,
                               key_peak_line_ptr, line_window_lines_ptr, trip_key_ptr, trip_line_ptr, trip_time_ptr, trip_entry_ptr, key_trip_begin_ptr, max_entries,
                               max_trips)
        totals = N.gx_windows_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_windows(self._h.ptr, text_ptr, size, both[0].array, both[0].n, both[1], self._windows_window(both, window), int(threshold),
                                           terms.array, terms.n, self._bucket_flags(weak_hash, all_digits), C.byref(keys), C.byref(out) if windows else None,
                                           C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._windows_totals(totals), counts, nl.value

    def _windows_host(self, device_call, n_lines_cap, parts, threshold, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap):
        """_group_host with the window arrays beside the key arrays, each sized by the number of lines: no more entries than lines, no
        more trips than entries.  The trip arrays are passed only with a threshold (threshold 0 has no trips: they come back empty)."""
        got = {}
        cap = max(1, n_lines_cap)
        trips = int(threshold) != 0

        def call(units, ucap, koff, first, lines, stats, line_key, mk):
            got.update(entry_line=np.zeros(cap, np.uint32), entry_key=np.zeros(cap, np.uint32), entry_time=np.zeros(cap, np.int64),
                       entry_window_lines=np.zeros(cap, np.uint32), entry_window_sum=np.zeros((cap, 4), np.uint64) if parts.has_values else None,
                       key_entry_begin=np.zeros(mk + 1, np.uint64), key_peak_lines=np.zeros(max(1, mk), np.uint32),
                       key_peak_line=np.full(max(1, mk), 0xFFFFFFFF, np.uint32), line_window_lines=np.zeros(cap, np.uint32),
                       trip_key=np.zeros(cap, np.uint32), trip_line=np.zeros(cap, np.uint32), trip_time=np.zeros(cap, np.int64),
                       trip_entry=np.zeros(cap, np.uint32), key_trip_begin=np.zeros(mk + 1, np.uint64))
            ptrs = [None if got[name] is None or (not trips and (name.startswith("trip_") or name == "key_trip_begin")) else got[name].ctypes.data
                    for name in self.WINDOW_OUTS]
            return device_call(units, ucap, koff, first, lines, stats, line_key, mk, *ptrs, n_lines_cap, n_lines_cap)
        res, rest = self._group_host(call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap)
        m, t, k = res["totals"]["entries"], res["totals"]["n_trips"], res["totals"]["n_keys"]
        ws = got["entry_window_sum"]
        res.update(entry_line=got["entry_line"][:m], entry_key=got["entry_key"][:m], entry_time=got["entry_time"][:m],
                   entry_window_lines=got["entry_window_lines"][:m], key_entry_begin=got["key_entry_begin"][:k + 1], key_peak_lines=got["key_peak_lines"][:k],
                   key_peak_line=got["key_peak_line"][:k], line_window_lines=got["line_window_lines"], trip_key=got["trip_key"][:t],
                   trip_line=got["trip_line"][:t], trip_time=got["trip_time"][:t], trip_entry=got["trip_entry"][:t], key_trip_begin=got["key_trip_begin"][:k + 1],
                   entry_window_sum=None if ws is None else [{"numbers": int(x[0]), "sum": (int(x[2].astype(np.int64)) << 64) + int(x[1])} for x in ws[:m]])
        return res, rest

    def group_windows(self, data, offsets, ids, rows, parts, window, threshold=0, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None,
                      weak_hash=False, all_digits=False):
        """gx_group_windows on host buffers: group_lines' keys, and for every entry of a key (its lines ordered by a captured time) the
        number of the key's lines within `window` before it, itself included -- Splunk's `streamstats time_window= count by`, fail2ban's
        findtime -- and the TRIPS: the entries at which that count reaches `threshold` from below (0: no trips).  parts: (extraction, key
        extractor, time extractor[, value extractor]) each (series_parts); window an int >= 0 in the time's own unit, or a text read as
        group_sessions reads max_gap; everything else as group_lines takes it.  Returns group_lines' dict plus entry_line, entry_key,
        entry_time, entry_window_lines, entry_window_sum (per entry, ordered by (key, time, line); the sums dicts of numbers and sum,
        None when no part has a value extractor), key_entry_begin (n_keys + 1), key_peak_lines, key_peak_line (per key; 0 and
        0xFFFFFFFF: no entry), line_window_lines (uint32 per input line, 0: no entry), trip_key, trip_line, trip_time, trip_entry (per
        trip, in the same order), key_trip_begin (n_keys + 1) and the window totals (entries, number_unset, not_numbers, n_trips,
        tripped_keys, peak_lines, peak_line, peak_key, first_time, last_time) in totals."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        both = self.series_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.group_windows_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), both, window, threshold, where, *outs,
                                             offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8),
                                             weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._windows_host(device_call, n, both[0], threshold, data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap)
        res["line_key"], res["line_window_lines"] = res["line_key"][:n], res["line_window_lines"][:n]
        return res

    def text_group_windows(self, text, parts, window, threshold=0, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None, weak_hash=False,
                           all_digits=False):
        """gx_text_group_windows on a host buffer: raw text -> lines -> extraction -> group_windows.  Returns (the dict group_windows
        returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        both = self.series_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.text_group_windows_device(raw.ctypes.data if raw.size else None, raw.size, both, window, threshold, where, *outs, device_pointers=False,
                                                  utf8=utf8, weak_hash=weak_hash, all_digits=all_digits)
        res, (counts, n_lines) = self._windows_host(device_call, cap_lines, both[0], threshold, np.uint8, np.uint32, keys, decode, max_keys, key_units_cap)
        res["line_key"], res["line_window_lines"] = res["line_key"][:n_lines], res["line_window_lines"][:n_lines]
        return res, counts, n_lines

    # -- begin/end spans per captured text: a key's start and end lines paired in input order (gx_group_spans / gx_text_group_spans) --
    SPAN_ROLES = {"begin": N.GX_SPAN_BEGIN, "end": N.GX_SPAN_END, N.GX_SPAN_BEGIN: N.GX_SPAN_BEGIN, N.GX_SPAN_END: N.GX_SPAN_END}

    def span_parts(self, spec):
        """Resolves a list of (extraction, key extractor, time extractor, role[, value extractor]) into (GroupParts, int32 number groups,
        uint32 roles): the first three and the optional fifth entry as series_parts takes a part (time None: the part's lines have a
        key and no time, -1), role "begin" / "end" (or GX_SPAN_BEGIN / GX_SPAN_END).  A (GroupParts, numbers, roles) tuple passes
        through."""
        if isinstance(spec, tuple) and len(spec) == 3 and isinstance(spec[0], GroupParts):
            return spec
        spec = [tuple(item) for item in spec]
        for item in spec:
            if len(item) not in (4, 5):
                raise ValueError("a part is (extraction, key extractor, time extractor, role[, value extractor])")
            if item[3] not in self.SPAN_ROLES:
                raise ValueError('role %r: "begin" or "end"' % (item[3],))
        parts, numbers = self.series_parts([item[:3] + tuple(item[4:]) for item in spec])
        roles = (C.c_uint32 * max(1, len(spec)))()
        for t, item in enumerate(spec):
            roles[t] = self.SPAN_ROLES[item[3]]
        return parts, numbers, roles

    @staticmethod
    def _stats_dict(x):
        return {"lines": x.lines, "numbers": x.numbers, "unset": x.unset, "not_numbers": x.not_numbers, "min": x.min if x.numbers else None,
                "max": x.max if x.numbers else None, "sum": (x.sum_hi << 64) + x.sum_lo}

    @staticmethod
    def _spans_totals(t):
        d = Gorp._group_totals(t.group)
        d.update(n_spans=t.n_spans, begins=t.begins, ends=t.ends, superseded=t.superseded, left_open=t.left_open, orphan_ends=t.orphan_ends,
                 out_of_range=t.out_of_range, durations=Gorp._stats_dict(t.durations), group=Gorp._group_totals(t.group))
        return d

    SPAN_OUTPUTS = ("span_key", "span_begin_line", "span_end_line", "span_begin", "span_end", "span_duration", "span_class", "key_span_begin", "key_span_stats",
                    "key_open_line", "line_span", "line_state")

    def group_spans_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                           key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, span_key_ptr=None,
                           span_begin_line_ptr=None, span_end_line_ptr=None, span_begin_ptr=None, span_end_ptr=None, span_duration_ptr=None, span_class_ptr=None,
                           key_span_begin_ptr=None, key_span_stats_ptr=None, key_open_line_ptr=None, line_span_ptr=None, line_state_ptr=None, max_spans=0,
                           spans=True, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False,
                           all_digits=False):
        """gx_group_spans on device pointers (ints): group_lines_device's keys, plus the spans in the caller's buffers, each optional
        (none at all: the size query; max_keys still sizes the table).  parts as span_parts takes them.  spans=False passes spans ==
        NULL: the call is gx_group_lines.  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says
        what the outputs need (n_keys, key_units, n_spans; keyed // 2 always suffices for max_spans); every other error raises."""
        three = self.span_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_spans_out(span_key_ptr, span_begin_line_ptr, span_end_line_ptr, span_begin_ptr, span_end_ptr, span_duration_ptr, span_class_ptr,
                             key_span_begin_ptr, key_span_stats_ptr, key_open_line_ptr, line_span_ptr, line_state_ptr, max_spans)
        totals = N.gx_spans_totals()
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (N.GX_BY_KEY_ALL_DIGITS if all_digits else 0)
        rc = N.lib().gx_group_spans(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, three[0].array, three[0].n, three[1], three[2], terms.array, terms.n,
                                    flags, C.byref(keys), C.byref(out) if spans else None, C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._spans_totals(totals)

    def text_group_spans_device(self, text_ptr, size, parts, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None, key_first_line_ptr=None,
                                key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, max_keys=0, span_key_ptr=None, span_begin_line_ptr=None,
                                span_end_line_ptr=None, span_begin_ptr=None, span_end_ptr=None, span_duration_ptr=None, span_class_ptr=None,
                                key_span_begin_ptr=None, key_span_stats_ptr=None, key_open_line_ptr=None, line_span_ptr=None, line_state_ptr=None, max_spans=0,
                                spans=True, offsets64=False, stream=None, device_pointers=True, utf8=False, weak_hash=False, all_digits=False):
        """gx_text_group_spans on a device buffer (int); outputs as group_spans_device takes them (line_key, line_span and line_state:
        one entry per line of the text).  Returns (rc, totals, counts, n_lines)."""
        three = self.span_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        keys = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        out = N.gx_spans_out(span_key_ptr, span_begin_line_ptr, span_end_line_ptr, span_begin_ptr, span_end_ptr, span_duration_ptr, span_class_ptr,
                             key_span_begin_ptr, key_span_stats_ptr, key_open_line_ptr, line_span_ptr, line_state_ptr, max_spans)
        totals = N.gx_spans_totals()
        nl = C.c_uint64(0)
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (N.GX_BY_KEY_ALL_DIGITS if all_digits else 0)
        rc = N.lib().gx_text_group_spans(self._h.ptr, text_ptr, size, three[0].array, three[0].n, three[1], three[2], terms.array, terms.n, flags, C.byref(keys),
                                         C.byref(out) if spans else None, C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):
            _check(rc)
        return rc, self._spans_totals(totals), counts, nl.value

    def _spans_host(self, device_call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap, max_spans):
        """_group_host with the span arrays beside the key arrays: the per-span ones sized by max_spans (None: half the lines, which
        always suffices; a smaller one is grown once to what the call reported), the per-line ones by the number of lines."""
        got = {}
        cap_lines = max(1, n_lines_cap)
        want = [n_lines_cap // 2 if max_spans is None else max_spans]

        def call(units, ucap, koff, first, lines, stats, line_key, mk):
            cap = max(1, want[0])
            got.update(span_key=np.zeros(cap, np.uint32), span_begin_line=np.zeros(cap, np.uint32), span_end_line=np.zeros(cap, np.uint32),
                       span_begin=np.zeros(cap, np.int64), span_end=np.zeros(cap, np.int64), span_duration=np.zeros(cap, np.int64),
                       span_class=np.zeros(cap, np.uint8), key_span_begin=np.zeros(mk + 1, np.uint64), key_span_stats=(N.gx_measure_stats * max(1, mk))(),
                       key_open_line=np.full(max(1, mk), 0xFFFFFFFF, np.uint32), line_span=np.full(cap_lines, 0xFFFFFFFF, np.uint32),
                       line_state=np.zeros(cap_lines, np.uint8))
            ptrs = [C.addressof(got[name]) if name == "key_span_stats" else got[name].ctypes.data for name in self.SPAN_OUTPUTS]
            ret = device_call(units, ucap, koff, first, lines, stats, line_key, mk, *ptrs, want[0])
            want[0] = max(want[0], ret[1]["n_spans"])
            return ret
        res, rest = self._group_host(call, n_lines_cap, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, key_units_cap)
        s, k = res["totals"]["n_spans"], res["totals"]["n_keys"]
        for name in self.SPAN_OUTPUTS[:7]:
            res[name] = got[name][:s]
        res.update(key_span_begin=got["key_span_begin"][:k + 1], key_span_stats=[self._stats_dict(x) for x in got["key_span_stats"][:k]],
                   key_open_line=got["key_open_line"][:k], line_span=got["line_span"], line_state=got["line_state"])
        return res, rest

    def group_spans(self, data, offsets, ids, rows, parts, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None, max_spans=None,
                    weak_hash=False, all_digits=False):
        """gx_group_spans on host buffers: group_lines' keys, and every key's BEGIN and END lines paired in input order -- Splunk's
        `transaction id startswith= endswith=`: an END forms a SPAN with the entry just before it among its key's lines if and only if
        that entry is a BEGIN.  parts: (extraction, key extractor, time extractor, "begin" | "end"[, value extractor]) each
        (span_parts; time None: no time); everything else as group_lines takes it.  Returns group_lines' dict plus span_key,
        span_begin_line, span_end_line, span_begin, span_end, span_duration, span_class (per span, ordered by (key number, end line);
        class 0 duration, 1 unset, 2 not a number), key_span_begin (n_keys + 1), key_span_stats and key_open_line (per key; 0xFFFFFFFF:
        no begin is left open), line_span (uint32 per input line, 0xFFFFFFFF: none), line_state (uint8 per input line: 0 no entry, 1 a
        span's begin, 2 a span's end, 3 a begin superseded, 4 a begin left open, 5 an end without a begin) and the span totals (n_spans,
        begins, ends, superseded, left_open, orphan_ends, out_of_range, durations) in totals."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        three = self.span_parts(parts)
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.group_spans_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), three, where, *outs, offsets64=offsets.dtype == np.uint64,
                                           utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8), weak_hash=weak_hash, all_digits=all_digits)
        res, _ = self._spans_host(device_call, n, three[0], data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap, max_spans)
        res["line_key"], res["line_span"], res["line_state"] = res["line_key"][:n], res["line_span"][:n], res["line_state"][:n]
        return res

    def text_group_spans(self, text, parts, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None, max_spans=None, weak_hash=False,
                         all_digits=False):
        """gx_text_group_spans on a host buffer: raw text -> lines -> extraction -> group_spans.  Returns (the dict group_spans returns,
        counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        three = self.span_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def device_call(*outs):
            return self.text_group_spans_device(raw.ctypes.data if raw.size else None, raw.size, three, where, *outs, device_pointers=False, utf8=utf8,
                                                weak_hash=weak_hash, all_digits=all_digits)
        res, (counts, n_lines) = self._spans_host(device_call, cap_lines, three[0], np.uint8, np.uint32, keys, decode, max_keys, key_units_cap, max_spans)
        res["line_key"], res["line_span"], res["line_state"] = res["line_key"][:n_lines], res["line_span"][:n_lines], res["line_state"][:n_lines]
        return res, counts, n_lines

    # -- percentiles of a captured number per captured text (gx_group_quantiles / gx_text_group_quantiles) ------------------------
    def group_quantiles_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, quantiles, where=None, key_units_ptr=None, key_units_cap=0,
                               key_offsets_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, key_quantiles_ptr=None,
                               max_keys=0, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_group_quantiles on device pointers (ints): group_lines_device plus key_quantiles_ptr, room for max_keys x len(quantiles)
        gx_quantile_out rows, key-major (optional).  quantiles: see quantile_asks.  Returns (rc, totals) as group_lines_device does."""
        parts = self.group_parts(parts)
        asks, n_q = self.quantile_asks(quantiles)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        totals = N.gx_group_totals()
        rc = N.lib().gx_group_quantiles(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, asks, n_q,
                                        N.GX_GROUP_WEAK_HASH if weak_hash else 0, C.byref(out), key_quantiles_ptr, C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._group_totals(totals)

    def text_group_quantiles_device(self, text_ptr, size, parts, quantiles, where=None, key_units_ptr=None, key_units_cap=0, key_offsets_ptr=None,
                                    key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_key_ptr=None, key_quantiles_ptr=None, max_keys=0,
                                    offsets64=False, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_text_group_quantiles on a device buffer (int); outputs as group_quantiles_device takes them.  Returns (rc, totals, counts,
        n_lines)."""
        parts = self.group_parts(parts)
        asks, n_q = self.quantile_asks(quantiles)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out = N.gx_group_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_key_ptr, max_keys)
        totals = N.gx_group_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_group_quantiles(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, asks, n_q,
                                             N.GX_GROUP_WEAK_HASH if weak_hash else 0, C.byref(out), key_quantiles_ptr, C.byref(totals), counts.ctypes.data,
                                             C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._group_totals(totals), counts, nl.value

    def group_quantiles(self, data, offsets, ids, rows, parts, quantiles, where=None, utf8=None, keys="list", max_keys=None, key_units_cap=None,
                        weak_hash=False):
        """gx_group_quantiles on host buffers: group_lines, and per key the nearest-rank quantiles of the numbers its lines captured
        (the part's value extractor).  Returns group_lines' dict plus "quantiles": per key, in the keys' order, a list with a dict value
        / rank / below / equal per quantile in input order (value None where the key has no numbers).  quantiles: see quantile_asks.
        The retry on GX_E_LIMIT is group_lines'."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.group_parts(parts)
        asks = self.quantile_asks(quantiles)
        pairs = [(asks[0][q].num, asks[0][q].den) for q in range(asks[1])]
        n = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, cap, koff, first, lines, stats, line_key, mk, kq):
            return self.group_quantiles_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), parts, pairs, where, units, cap, koff, first, lines, stats,
                                               line_key, kq, mk, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False,
                                               utf8=bool(utf8), weak_hash=weak_hash)
        res, _ = self._group_host(call, n, parts, data.dtype, offsets.dtype, keys, decode, max_keys, key_units_cap, n_q=len(pairs))
        res["line_key"] = res["line_key"][:n]
        return res

    def text_group_quantiles(self, text, parts, quantiles, where=None, utf8=False, keys="list", max_keys=None, key_units_cap=None):
        """gx_text_group_quantiles on a host buffer: raw text -> lines -> extraction -> group_quantiles.  Returns (the dict
        group_quantiles returns, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.group_parts(parts)
        asks = self.quantile_asks(quantiles)
        pairs = [(asks[0][q].num, asks[0][q].den) for q in range(asks[1])]
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, cap, koff, first, lines, stats, line_key, mk, kq):
            return self.text_group_quantiles_device(raw.ctypes.data if raw.size else None, raw.size, parts, pairs, where, units, cap, koff, first, lines, stats,
                                                    line_key, kq, mk, device_pointers=False, utf8=utf8)
        res, (counts, n_lines) = self._group_host(call, cap_lines, parts, np.uint8, np.uint32, keys, decode, max_keys, key_units_cap, n_q=len(pairs))
        res["line_key"] = res["line_key"][:n_lines]
        return res, counts, n_lines

    # -- keys ranked by their lines or numbers (gx_top_groups / gx_text_top_groups) ------------------------------------------------
    RANK_BY = {"lines": N.GX_RANK_LINES, "numbers": N.GX_RANK_NUMBERS, "sum": N.GX_RANK_SUM, "max": N.GX_RANK_MAX, "min": N.GX_RANK_MIN}

    @staticmethod
    def _top_groups_totals(t):
        return {"group": Gorp._group_totals(t.group), "candidates": t.candidates, "n_top": t.n_top, "units_top": t.units_top,
                "last": (t.last_hi << 64) + t.last_lo if t.n_top else None, "ties_left": t.ties_left}

    @staticmethod
    def _rank_by(by):
        if by not in Gorp.RANK_BY:
            raise ValueError('by: "lines", "numbers", "sum", "max" or "min"')
        return Gorp.RANK_BY[by]

    def top_groups_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts, n_wanted, by="lines", largest=True, where=None, key_units_ptr=None,
                          key_units_cap=0, key_offsets_ptr=None, key_number_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None,
                          line_rank_ptr=None, cap_keys=0, max_keys=0, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False,
                          weak_hash=False):
        """gx_top_groups on device pointers (ints); the outputs are the caller's buffers, each optional (none at all: the size query;
        max_keys still sizes the table).  Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says
        what the outputs need (n_top, units_top; group.exact False: the table overflowed, max_keys = n always suffices); every other
        error raises."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_top_groups_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_number_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_rank_ptr,
                                  cap_keys)
        totals = N.gx_top_groups_totals()
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (0 if largest else N.GX_TOP_GROUPS_SMALLEST)
        rc = N.lib().gx_top_groups(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, self._rank_by(by),
                                   n_wanted, max_keys, flags, C.byref(out), C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._top_groups_totals(totals)

    def text_top_groups_device(self, text_ptr, size, parts, n_wanted, by="lines", largest=True, where=None, key_units_ptr=None, key_units_cap=0,
                               key_offsets_ptr=None, key_number_ptr=None, key_first_line_ptr=None, key_lines_ptr=None, key_stats_ptr=None, line_rank_ptr=None,
                               cap_keys=0, max_keys=0, offsets64=False, stream=None, device_pointers=True, utf8=False, weak_hash=False):
        """gx_text_top_groups on a device buffer (int); outputs as top_groups_device takes them (line_rank: one entry per line of the
        text).  Returns (rc, totals, counts, n_lines)."""
        parts = self.group_parts(parts)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out = N.gx_top_groups_out(key_units_ptr, key_units_cap, key_offsets_ptr, key_number_ptr, key_first_line_ptr, key_lines_ptr, key_stats_ptr, line_rank_ptr,
                                  cap_keys)
        totals = N.gx_top_groups_totals()
        nl = C.c_uint64(0)
        flags = (N.GX_GROUP_WEAK_HASH if weak_hash else 0) | (0 if largest else N.GX_TOP_GROUPS_SMALLEST)
        rc = N.lib().gx_text_top_groups(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, self._rank_by(by), n_wanted, max_keys, flags,
                                        C.byref(out), C.byref(totals), counts.ctypes.data, C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.group.n_keys):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._top_groups_totals(totals), counts, nl.value

    def _top_groups_host(self, call, n_lines_cap, n_wanted, parts, unit_dtype, offsets_dtype, keys, decode, max_keys, want_line_rank):
        """Runs `call(out arrays..., cap_keys, max_keys)` on host arrays; on GX_E_LIMIT once more with the units it reported, or -- when
        the table overflowed -- with max_keys = the number of lines: three calls at the most.  Builds the result dict."""
        max_keys = min(n_lines_cap, 1024) if max_keys is None else max_keys
        cap = max(1, n_wanted)
        key_units_cap = 65536
        for attempt in range(3):
            units = np.zeros(max(1, key_units_cap), unit_dtype)
            koff = np.zeros(cap + 1, offsets_dtype)
            number = np.zeros(cap, np.uint32)
            first = np.zeros(cap, np.uint32)
            lines = np.zeros(cap, np.uint64)
            stats = (N.gx_measure_stats * cap)() if parts.has_values else None
            line_rank = np.full(max(1, n_lines_cap), 0xFFFFFFFF, np.uint32) if want_line_rank else None
            got = call(units.ctypes.data, key_units_cap, koff.ctypes.data, number.ctypes.data, first.ctypes.data, lines.ctypes.data,
                       None if stats is None else C.addressof(stats), None if line_rank is None else line_rank.ctypes.data, cap, max_keys)
            rc, totals = got[0], got[1]
            if rc == N.GX_OK:
                break
            if attempt == 2:
                raise GorpError(rc, N.last_error())
            if totals["group"]["exact"]:
                key_units_cap = max(key_units_cap, totals["units_top"])
            else:
                max_keys = n_lines_cap
        k = totals["n_top"]
        koff, units = koff[:k + 1], units[:totals["units_top"]]
        res = {"key_units": units, "key_offsets": koff, "key_number": number[:k], "first_line": first[:k], "lines": lines[:k], "totals": totals,
               "stats": None if stats is None else [{"lines": s.lines, "numbers": s.numbers, "unset": s.unset, "not_numbers": s.not_numbers,
                                                      "min": s.min if s.numbers else None, "max": s.max if s.numbers else None,
                                                      "sum": (s.sum_hi << 64) + s.sum_lo} for s in stats[:k]]}
        if want_line_rank:
            res["line_rank"] = line_rank
        if keys == "list":
            res["keys"] = [decode(units[int(koff[j]):int(koff[j + 1])]) for j in range(k)]
        elif keys != "csr":
            raise ValueError('keys: "list" or "csr"')
        return res, got[2:]

    def top_groups(self, data, offsets, ids, rows, parts, n, by="lines", largest=True, where=None, utf8=None, keys="list", max_keys=None, line_rank=False,
                   weak_hash=False):
        """gx_top_groups on host buffers: the n keys (at most 4096) that rank highest -- lowest with largest=False -- by their lines, or
        by the numbers, sum, max or min of what the part's value extractor captured on their lines; ties go to the key that appeared
        first.  data / offsets / ids / rows, parts, where and utf8 as group_lines takes them.  Returns group_lines' dict shape in RANK
        order -- keys (keys="csr": left out), key_units / key_offsets, first_line, lines, stats -- plus key_number (the key's number
        in group_lines' order), line_rank with line_rank=True (uint32 per input line, 0xFFFFFFFF: no key, or its key not delivered),
        and totals: group (group_lines' totals), candidates, n_top, units_top, last (the rank value of the last delivered key as one
        int, None without one) and ties_left."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.group_parts(parts)
        n_lines = len(offsets) - 1
        decode = (lambda u: u.tobytes().decode("utf-16-le", "surrogatepass")) if utf16 else (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, ucap, koff, number, first, lines, stats, lrank, cap, mk):
            return self.top_groups_device(ptr(data), offsets.ctypes.data, n_lines, ptr(ids), ptr(caps), parts, n, by, largest, where, units, ucap, koff, number, first,
                                          lines, stats, lrank, cap, mk, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact,
                                          device_pointers=False, utf8=bool(utf8), weak_hash=weak_hash)
        res, _ = self._top_groups_host(call, n_lines, n, parts, data.dtype, offsets.dtype, keys, decode, max_keys, line_rank)
        if line_rank:
            res["line_rank"] = res["line_rank"][:n_lines]
        return res

    def text_top_groups(self, text, parts, n, by="lines", largest=True, where=None, utf8=False, keys="list", max_keys=None, line_rank=False):
        """gx_text_top_groups on a host buffer: raw text -> lines -> extraction -> top_groups.  Returns (the dict top_groups returns,
        counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.group_parts(parts)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        decode = (lambda u: u.tobytes().decode("utf-8")) if utf8 else (lambda u: u.tobytes())

        def call(units, ucap, koff, number, first, lines, stats, lrank, cap, mk):
            return self.text_top_groups_device(raw.ctypes.data if raw.size else None, raw.size, parts, n, by, largest, where, units, ucap, koff, number, first, lines,
                                               stats, lrank, cap, mk, device_pointers=False, utf8=utf8)
        res, (counts, n_lines) = self._top_groups_host(call, cap_lines, n, parts, np.uint8, np.uint32, keys, decode, max_keys, line_rank)
        if line_rank:
            res["line_rank"] = res["line_rank"][:n_lines]
        return res, counts, n_lines

    # -- lines ranked by a number they captured (gx_top_lines / gx_text_top_lines) ------------------------------------------------
    def top_parts(self, spec):
        """Resolves a list of (extraction, value extractor) into gx_top_part records: extraction is a name or an index, the extractor a
        name or a group index (a name two groups of the extraction share is a ValueError).  At most one part per extraction, at most
        64 parts; all parts share one number space.  Returns a TopParts; a TopParts passes through."""
        if isinstance(spec, TopParts):
            return spec
        spec = list(spec)
        if len(spec) > 64:
            raise ValueError("at most 64 parts")
        arr = (N.gx_top_part * max(1, len(spec)))()
        seen = set()
        for t, item in enumerate(spec):
            item = tuple(item)
            if len(item) != 2:
                raise ValueError("a part is (extraction, value extractor)")
            k, g = self._extraction_and_group(item[0], item[1])
            if k in seen:
                raise ValueError("two parts for extraction %r" % (item[0],))
            seen.add(k)
            arr[t].extraction, arr[t].value_group = k, g
        return TopParts(arr, len(spec))

    @staticmethod
    def _top_totals(t):
        return {"lines": t.lines, "numbers": t.numbers, "unset": t.unset, "not_numbers": t.not_numbers, "n_top": t.n_top, "units_top": t.units_top,
                "last_value": t.last_value, "ties_left": t.ties_left}

    def top_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, by, n_wanted, largest=True, where=None, out_index_ptr=None, out_values_ptr=None,
                         out_data_ptr=None, out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0, offsets64=False,
                         utf16=False, compact=0, stream=None, device_pointers=True, utf8=False):
        """gx_top_lines on device pointers (ints); the outputs are the caller's buffers, each optional (none at all: the size query).
        Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says what the outputs need (n_top,
        units_top); every other error raises."""
        parts = self.top_parts(by)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        totals = N.gx_top_totals()
        rc = N.lib().gx_top_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, n_wanted,
                                  0 if largest else N.GX_TOP_SMALLEST, out_index_ptr, out_values_ptr, out_data_ptr, out_offsets_ptr, out_ids_ptr, out_caps_ptr,
                                  cap_lines, out_bytes_cap, C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_top):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._top_totals(totals)

    def top_lines(self, data, offsets, ids, rows, by, n, largest=True, where=None, utf8=None):
        """gx_top_lines on host buffers: the n lines that captured the largest numbers (largest=False: the smallest), ordered by (value,
        input line); ties at the cut go to the earliest lines.  by: Gorp.top_parts or its input, one (extraction, value extractor) per
        extraction that takes part; where: terms as capture_stats takes them.  data / offsets / ids / rows and utf8 as capture_stats
        takes them.  Makes the size query first and then the call.  Returns (index, values, data2, offsets2, ids2, rows2, totals): the
        delivered lines' input line numbers (uint32), their numbers (int64), the lines as a CSR batch with their ids and rows (rows2
        None without dense rows), and totals (lines, numbers, unset, not_numbers, n_top, units_top, last_value, ties_left)."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.top_parts(by)
        nl = len(offsets) - 1
        args = dict(largest=largest, where=where, offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8))
        _, totals = self.top_lines_device(ptr(data), offsets.ctypes.data, nl, ptr(ids), ptr(caps), parts, n, **args)
        k, units = totals["n_top"], totals["units_top"]
        index = np.zeros(max(1, k), np.uint32)
        values = np.zeros(max(1, k), np.int64)
        out = np.zeros(max(1, units), data.dtype)
        out_off = np.zeros(k + 1, offsets.dtype)
        out_ids = np.zeros((max(1, k),) + ids.shape[1:], ids.dtype)
        out_caps = None if caps is None else np.zeros((max(1, k), 2 * self.max_groups), np.int32)
        rc, totals = self.top_lines_device(ptr(data), offsets.ctypes.data, nl, ptr(ids), ptr(caps), parts, n, out_index_ptr=index.ctypes.data,
                                           out_values_ptr=values.ctypes.data, out_data_ptr=out.ctypes.data, out_offsets_ptr=out_off.ctypes.data,
                                           out_ids_ptr=out_ids.ctypes.data, out_caps_ptr=None if out_caps is None else out_caps.ctypes.data,
                                           cap_lines=k, out_bytes_cap=units * data.itemsize, **args)
        if rc != N.GX_OK:
            raise GorpError(rc, N.last_error())
        return index[:k], values[:k], out[:units], out_off, out_ids[:k], None if out_caps is None else out_caps[:k], totals

    def text_top_lines_device(self, text_ptr, size, by, n_wanted, largest=True, where=None, out_index_ptr=None, out_values_ptr=None, out_ptr=None, out_cap=0,
                              stream=None, device_pointers=True, utf8=False):
        """gx_text_top_lines on a device buffer (int): out_index_ptr / out_values_ptr have room for n_wanted entries, out_ptr for out_cap
        bytes; all None: the size query.  Returns (rc, totals, out_size, counts, n_lines); rc as top_lines_device returns it."""
        parts = self.top_parts(by)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        totals = N.gx_top_totals()
        out_size, nl = C.c_uint64(0), C.c_uint64(0)
        rc = N.lib().gx_text_top_lines(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, n_wanted, 0 if largest else N.GX_TOP_SMALLEST,
                                       out_index_ptr, out_values_ptr, out_ptr, out_cap, C.byref(out_size), C.byref(totals), counts.ctypes.data, C.byref(nl),
                                       C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.n_top):
            _check(rc)
        return rc, self._top_totals(totals), out_size.value, counts, nl.value

    def text_top_lines(self, text, by, n, largest=True, where=None, utf8=False):
        """gx_text_top_lines on a host buffer: raw text -> lines -> extraction -> top_lines.  Returns (index, values, the delivered
        lines' text as bytes -- each with its terminator, in rank order --, totals, counts uint64[2K + 2] of outcomes, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        ptr = raw.ctypes.data if raw.size else None
        parts = self.top_parts(by)
        _, totals, size, _, _ = self.text_top_lines_device(ptr, raw.size, parts, n, largest, where, device_pointers=False, utf8=utf8)
        index = np.zeros(max(1, n), np.uint32)
        values = np.zeros(max(1, n), np.int64)
        out = np.zeros(max(1, size), np.uint8)
        rc, totals, size, counts, n_lines = self.text_top_lines_device(ptr, raw.size, parts, n, largest, where, index.ctypes.data, values.ctypes.data,
                                                                       out.ctypes.data, size, device_pointers=False, utf8=utf8)
        if rc != N.GX_OK:
            raise GorpError(rc, N.last_error())
        k = totals["n_top"]
        return index[:k], values[:k], out[:size].tobytes(), totals, counts, n_lines

    # -- a whole batch ordered by a number its lines captured (gx_sort_lines / gx_text_sort_lines) ---------------------------------
    @staticmethod
    def _sort_totals(t):
        return {"lines": t.lines, "numbers": t.numbers, "unset": t.unset, "not_numbers": t.not_numbers, "carried": t.carried, "rest": t.rest,
                "lines_out": t.lines_out, "units_out": t.units_out, "first_value": t.first_value, "last_value": t.last_value, "n_passes": t.n_passes,
                "already_ordered": bool(t.already_ordered)}

    @staticmethod
    def _sort_flags(descending, carry, rest, all_digits):
        if rest not in ("drop", "last"):
            raise ValueError('rest: "drop" or "last"')
        return ((N.GX_SORT_DESCENDING if descending else 0) | (N.GX_SORT_CARRY if carry else 0) | (N.GX_SORT_REST_LAST if rest == "last" else 0)
                | (N.GX_SORT_ALL_DIGITS if all_digits else 0))

    def sort_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, by, descending=False, carry=False, rest="drop", where=None, out_index_ptr=None,
                          out_values_ptr=None, out_class_ptr=None, out_data_ptr=None, out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0,
                          out_bytes_cap=0, offsets64=False, utf16=False, compact=0, stream=None, device_pointers=True, utf8=False, all_digits=False):
        """gx_sort_lines on device pointers (ints); the outputs are the caller's buffers, each optional (none at all: the size query).
        Returns (rc, totals): rc is GX_OK or GX_E_LIMIT -- then nothing was written and totals says what the outputs need (lines_out,
        units_out); every other error raises."""
        parts = self.top_parts(by)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = N.gx_sort_out(out_index_ptr, out_values_ptr, out_class_ptr, out_data_ptr, out_offsets_ptr, out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap)
        totals = N.gx_sort_totals()
        rc = N.lib().gx_sort_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n,
                                   self._sort_flags(descending, carry, rest, all_digits), C.byref(out), C.byref(totals), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.lines_out):   # (a capacity's GX_E_LIMIT says what is needed; a refusal's says nothing)
            _check(rc)
        return rc, self._sort_totals(totals)

    def sort_lines(self, data, offsets, ids, rows, by, descending=False, carry=False, rest="drop", where=None, utf8=None, all_digits=False):
        """gx_sort_lines on host buffers: the batch ordered by (the number a line captured, input line) -- two hosts' logs as one
        timeline.  by: Gorp.top_parts or its input, one (extraction, value extractor) per extraction that takes part; where: terms as
        capture_stats takes them; data / offsets / ids / rows and utf8 as capture_stats takes them.  carry: a line without a number of
        its own travels with the nearest earlier line that has one (stack traces kept with their line); rest: the remaining lines are
        dropped ("drop") or follow in input order ("last").  Returns a dict: index (input line of every output line, uint32), values
        (int64; a carried line's is its header's, a rest line's 0), line_class (uint8: 0 own number, 1 carried, 2 rest), data / offsets
        (the lines as a CSR batch), ids and caps (their ids or whole rows; caps None for compact rows or without rows) and totals."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        parts = self.top_parts(by)
        n = len(offsets) - 1
        total = int(offsets[n] - offsets[0]) if n else 0
        # no ordering is larger than its input
        index = np.zeros(max(1, n), np.uint32)
        values = np.zeros(max(1, n), np.int64)
        line_class = np.zeros(max(1, n), np.uint8)
        out = np.zeros(max(1, total), data.dtype)
        out_off = np.zeros(n + 1, offsets.dtype)
        out_ids = np.zeros((max(1, n),) + ids.shape[1:], ids.dtype)
        out_caps = None if caps is None else np.zeros((max(1, n), 2 * self.max_groups), np.int32)
        rc, totals = self.sort_lines_device(ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), parts, descending, carry, rest, where,
                                            out_index_ptr=index.ctypes.data, out_values_ptr=values.ctypes.data, out_class_ptr=line_class.ctypes.data,
                                            out_data_ptr=out.ctypes.data, out_offsets_ptr=out_off.ctypes.data, out_ids_ptr=out_ids.ctypes.data,
                                            out_caps_ptr=None if out_caps is None else out_caps.ctypes.data, cap_lines=n, out_bytes_cap=total * data.itemsize,
                                            offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8),
                                            all_digits=all_digits)
        if rc != N.GX_OK:
            raise GorpError(rc, N.last_error())
        m = totals["lines_out"]
        return {"index": index[:m], "values": values[:m], "line_class": line_class[:m], "data": out[:totals["units_out"]], "offsets": out_off[:m + 1],
                "ids": out_ids[:m], "caps": None if out_caps is None else out_caps[:m], "totals": totals}

    def text_sort_lines_device(self, text_ptr, size, by, descending=False, carry=False, rest="drop", where=None, out_ptr=None, out_cap=0, out_offsets_ptr=None,
                               out_index_ptr=None, out_values_ptr=None, out_class_ptr=None, stream=None, device_pointers=True, utf8=False, all_digits=False):
        """gx_text_sort_lines on a device buffer (int); out_offsets (uint32), out_index, out_values and out_class are sized by the size
        query (all outputs None).  Returns (rc, totals, counts, n_lines); rc as sort_lines_device returns it."""
        parts = self.top_parts(by)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        totals = N.gx_sort_totals()
        nl = C.c_uint64(0)
        rc = N.lib().gx_text_sort_lines(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, self._sort_flags(descending, carry, rest, all_digits),
                                        out_ptr, out_cap, out_offsets_ptr, out_index_ptr, out_values_ptr, out_class_ptr, C.byref(totals), counts.ctypes.data,
                                        C.byref(nl), C.byref(o))
        if not (rc == N.GX_E_LIMIT and totals.lines_out):
            _check(rc)
        return rc, self._sort_totals(totals), counts, nl.value

    def text_sort_lines(self, text, by, descending=False, carry=False, rest="drop", where=None, utf8=False, all_digits=False):
        """gx_text_sort_lines on a host buffer: raw text -> lines -> extraction -> sort_lines.  Returns (the dict sort_lines returns
        without ids and caps: data holds the delivered lines' original bytes, each with its terminator, offsets (uint32) delimits them,
        index holds line numbers of the text; counts uint64[2K + 2] of outcomes; n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        parts = self.top_parts(by)
        cap_lines = int(np.count_nonzero(raw == 10)) + int(np.count_nonzero(raw == 13)) + 1   # (no more lines than line ends, plus the last)
        index = np.zeros(cap_lines, np.uint32)
        values = np.zeros(cap_lines, np.int64)
        line_class = np.zeros(cap_lines, np.uint8)
        out = np.zeros(max(1, raw.size), np.uint8)
        out_off = np.zeros(cap_lines + 1, np.uint32)
        rc, totals, counts, n_lines = self.text_sort_lines_device(raw.ctypes.data if raw.size else None, raw.size, parts, descending, carry, rest, where,
                                                                  out.ctypes.data, raw.size, out_off.ctypes.data, index.ctypes.data, values.ctypes.data,
                                                                  line_class.ctypes.data, device_pointers=False, utf8=utf8, all_digits=all_digits)
        if rc != N.GX_OK:
            raise GorpError(rc, N.last_error())
        m = totals["lines_out"]
        return ({"index": index[:m], "values": values[:m], "line_class": line_class[:m], "data": out[:totals["units_out"]], "offsets": out_off[:m + 1],
                 "totals": totals}, counts, n_lines)

    # -- percentiles of a number the lines captured (gx_capture_quantiles / gx_text_capture_quantiles) -------------------------------
    @staticmethod
    def quantile_asks(quantiles):
        """Resolves quantiles into gx_quantile records (num, den): a quantile is a pair (num, den) taken as it is, a
        fractions.Fraction, an int 0 or 1, or a float or decimal string taken at its decimal face value (Fraction(repr(q)): 0.99 is
        99/100).  A quantile outside [0, 1], a denominator of 0 or beyond 32 bits, or more than 16 of them: GorpError, before the
        library is called.  Returns (array, n)."""
        quantiles = list(quantiles)
        if len(quantiles) > N.GX_QUANTILE_MAX:
            raise GorpError(N.GX_E_LIMIT, "at most %d quantiles" % N.GX_QUANTILE_MAX)
        arr = (N.gx_quantile * max(1, len(quantiles)))()
        for t, q in enumerate(quantiles):
            if isinstance(q, bool):
                raise GorpError(N.GX_E_ARG, "a quantile is (num, den), a Fraction, a float or a decimal string: %r" % (q,))
            if isinstance(q, (tuple, list)):
                if len(q) != 2 or any(isinstance(x, bool) or not isinstance(x, (int, np.integer)) for x in q):
                    raise GorpError(N.GX_E_ARG, "a quantile pair is (num, den) in integers: %r" % (q,))
                num, den = int(q[0]), int(q[1])
            else:
                try:
                    f = Fraction(repr(float(q))) if isinstance(q, float) else Fraction(q)
                except (ValueError, TypeError, ZeroDivisionError):
                    raise GorpError(N.GX_E_ARG, "not a quantile: %r" % (q,))
                num, den = f.numerator, f.denominator
            if den < 1 or num < 0 or num > den:
                raise GorpError(N.GX_E_ARG, "a quantile lies in [0, 1]: %r" % (q,))
            if den > 0xFFFFFFFF:
                raise GorpError(N.GX_E_LIMIT, "a quantile's denominator has at most 32 bits: %r" % (q,))
            arr[t].num, arr[t].den = num, den
        return arr, len(quantiles)

    @staticmethod
    def _quantile_results(out, n_q, t):
        totals = {"lines": t.lines, "numbers": t.numbers, "unset": t.unset, "not_numbers": t.not_numbers}
        some = t.numbers != 0
        return [{"value": out[q].value if some else None, "rank": out[q].rank, "below": out[q].below, "equal": out[q].equal} for q in range(n_q)], totals

    def capture_quantiles_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, by, quantiles, where=None, offsets64=False, utf16=False, compact=0,
                                 stream=None, device_pointers=True, utf8=False):
        """gx_capture_quantiles on device pointers (ints).  Returns (results, totals): per quantile, in input order, a dict value / rank /
        below / equal (value None when there are no numbers), and totals (lines, numbers, unset, not_numbers)."""
        parts = self.top_parts(by)
        asks, n_q = self.quantile_asks(quantiles)
        terms = self.where_terms([] if where is None else where, units="utf-16" if utf16 else "utf-8" if utf8 else "latin-1")
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.utf8 = 1 if utf8 else 0
        o.compact_results = int(compact)
        o.stream = stream
        out = (N.gx_quantile_out * max(1, n_q))()
        totals = N.gx_quantile_totals()
        _check(N.lib().gx_capture_quantiles(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, parts.array, parts.n, terms.array, terms.n, asks, n_q, out,
                                            C.byref(totals), C.byref(o)))
        return self._quantile_results(out, n_q, totals)

    def capture_quantiles(self, data, offsets, ids, rows, by, quantiles, where=None, utf8=None):
        """gx_capture_quantiles on host buffers: nearest-rank quantiles -- sorted(values)[ceil(q * numbers) - 1] -- of the numbers the
        lines captured.  by: Gorp.top_parts or its input; quantiles: see quantile_asks; where: terms as capture_stats takes them.
        data / offsets / ids / rows and utf8 as capture_stats takes them.  Returns what capture_quantiles_device returns."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        if utf8 not in (None, False, "bytes"):
            raise ValueError('utf8: None or "bytes" (values are read in the units the offsets count)')
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        return self.capture_quantiles_device(ptr(data), offsets.ctypes.data, len(offsets) - 1, ptr(ids), ptr(caps), by, quantiles, where=where,
                                             offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False, utf8=bool(utf8))

    def text_capture_quantiles_device(self, text_ptr, size, by, quantiles, where=None, stream=None, device_pointers=True, utf8=False):
        """gx_text_capture_quantiles on a device buffer (int).  Returns (results, totals, counts uint64[2K + 2] of outcomes, n_lines)."""
        parts = self.top_parts(by)
        asks, n_q = self.quantile_asks(quantiles)
        terms = self.where_terms([] if where is None else where, units="utf-8" if utf8 else "latin-1")
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out = (N.gx_quantile_out * max(1, n_q))()
        totals = N.gx_quantile_totals()
        nl = C.c_uint64(0)
        _check(N.lib().gx_text_capture_quantiles(self._h.ptr, text_ptr, size, parts.array, parts.n, terms.array, terms.n, asks, n_q, out, C.byref(totals),
                                                 counts.ctypes.data, C.byref(nl), C.byref(o)))
        results, totals = self._quantile_results(out, n_q, totals)
        return results, totals, counts, nl.value

    def text_capture_quantiles(self, text, by, quantiles, where=None, utf8=False):
        """gx_text_capture_quantiles on a host buffer: raw text -> lines -> extraction -> capture_quantiles.  Returns (results, totals,
        counts, n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        return self.text_capture_quantiles_device(raw.ctypes.data if raw.size else None, raw.size, by, quantiles, where, device_pointers=False, utf8=utf8)

    def partition_lines(self, data, offsets, ids, rows=None, want=None):
        """gx_partition_lines on host buffers: the kept lines of the CSR batch ordered by (outcome index, input line number) -- every
        sink's lines at once.  want: as for select_lines, or None = every outcome 0 .. 2K.  Returns what select_lines returns plus
        group_lines, group_units (uint64[2K + 3]): outcome x's lines are out_offsets[group_lines[x] : group_lines[x + 1] + 1], its code
        units data[group_units[x] : group_units[x + 1]]."""
        utf16 = getattr(data, "dtype", None) == np.uint16
        data = np.ascontiguousarray(data, dtype=np.uint16 if utf16 else np.uint8)
        offsets = np.ascontiguousarray(offsets)
        if offsets.dtype not in (np.uint32, np.uint64):
            raise TypeError("offsets must be uint32 or uint64")
        ids = np.ascontiguousarray(ids)
        compact = self._ids_format(ids)
        n = len(offsets) - 1
        caps = None if rows is None or compact else np.ascontiguousarray(rows, dtype=np.int32)
        ptr = lambda a: a.ctypes.data if a is not None and a.size else None
        args = dict(offsets64=offsets.dtype == np.uint64, utf16=utf16, compact=compact, device_pointers=False)
        # one pass: no partition is larger than its input
        total = int(offsets[n] - offsets[0]) if n else 0
        index = np.zeros(n, np.uint32)
        out = np.zeros(total, data.dtype)
        out_off = np.zeros(n + 1, offsets.dtype)
        out_ids = np.zeros(ids.shape, ids.dtype)
        out_caps = None if caps is None else np.zeros((n, 2 * self.max_groups), np.int32)
        k, nbytes, group_lines, group_units = self.partition_lines_device(
            ptr(data), offsets.ctypes.data, n, ptr(ids), ptr(caps), want, out_index_ptr=index.ctypes.data, out_data_ptr=out.ctypes.data,
            out_offsets_ptr=out_off.ctypes.data, out_ids_ptr=out_ids.ctypes.data, out_caps_ptr=None if out_caps is None else out_caps.ctypes.data,
            cap_lines=n, out_bytes_cap=total * data.itemsize, **args)
        index, out, out_off, out_ids = index[:k], out[:nbytes // data.itemsize], out_off[:k + 1], out_ids[:k]
        out_caps = None if out_caps is None else out_caps[:k]
        if compact:
            return index, out, out_off, out_ids, group_lines, group_units
        if caps is not None:
            return index, out, out_off, out_ids, out_caps, group_lines, group_units
        return index, out, out_off, group_lines, group_units

    def partition_lines_device(self, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, want=None, out_index_ptr=None, out_data_ptr=None,
                               out_offsets_ptr=None, out_ids_ptr=None, out_caps_ptr=None, cap_lines=0, out_bytes_cap=0, offsets64=False,
                               utf16=False, compact=0, stream=None, no_sync=False, device_pointers=True):
        """gx_partition_lines on device pointers (ints); every output optional, none at all only asks for the sizes and the groups.
        want=None keeps every outcome 0 .. 2K.  Returns (lines, bytes, group_lines, group_units).  GorpError with code GX_E_LIMIT when
        a capacity is too small."""
        mask = None if want is None else self.want_mask(want)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.offsets64 = 1 if offsets64 else 0
        o.utf16 = 1 if utf16 else 0
        o.compact_results = int(compact)
        o.stream = stream
        o.no_sync = 1 if no_sync else 0
        k, nbytes = C.c_uint64(0), C.c_uint64(0)
        group_lines = np.zeros(2 * self.num_extractions + 3, np.uint64)
        group_units = np.zeros(2 * self.num_extractions + 3, np.uint64)
        _check(N.lib().gx_partition_lines(self._h.ptr, data_ptr, offsets_ptr, n, ids_ptr, caps_ptr, None if mask is None else mask.ctypes.data,
                                          out_index_ptr, out_data_ptr, out_offsets_ptr, out_ids_ptr, out_caps_ptr, cap_lines, out_bytes_cap,
                                          group_lines.ctypes.data, group_units.ctypes.data, C.byref(k), C.byref(nbytes), C.byref(o)))
        return k.value, nbytes.value, group_lines, group_units

    def text_to_jsonl_by_extraction(self, text, id_as=None, utf8=False):
        """gx_text_to_jsonl_by_extraction on a host buffer: raw log text -> the JSON Lines of text_to_jsonl regrouped stably by extraction.
        Returns (jsonl bytes, group_out uint64[K + 1], counts uint64[2K + 2], n_lines): extraction k's objects are
        jsonl[group_out[k] : group_out[k + 1]]."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        ptr = raw.ctypes.data if raw.size else None
        size = self.text_to_jsonl_by_extraction_device(ptr, raw.size, None, 0, id_as=id_as, utf8=utf8, device_pointers=False)[0]
        out = np.zeros(max(1, size), np.uint8)
        size, group_out, counts, n_lines = self.text_to_jsonl_by_extraction_device(ptr, raw.size, out.ctypes.data, size, id_as=id_as, utf8=utf8,
                                                                                   device_pointers=False)
        return out[:size].tobytes(), group_out, counts, n_lines

    def text_to_jsonl_by_extraction_device(self, text_ptr, size, out_ptr, out_cap, id_as=None, utf8_passthrough=False, stream=None, utf8=False,
                                           device_pointers=True):
        """gx_text_to_jsonl_by_extraction on device buffers (ints); out_ptr=None only asks for the sizes.
        Returns (text size, group_out, counts, n_lines)."""
        self._send_meta()
        K = self.num_extractions
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.utf8_passthrough = 1 if utf8_passthrough else 0
        o.utf8 = 1 if utf8 else 0
        o.stream = stream
        group_out = np.zeros(K + 1, np.uint64)
        counts = np.zeros(2 * K + 2, np.uint64)
        size_out, nl = C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_text_to_jsonl_by_extraction(self._h.ptr, text_ptr, size, id_as.encode("utf-8") if id_as is not None else None, out_ptr,
                                                      out_cap, C.byref(size_out), group_out.ctypes.data, counts.ctypes.data, C.byref(nl),
                                                      C.byref(o)))
        return size_out.value, group_out, counts, nl.value

    def text_select(self, text, want=("unmatched", "exceptions"), utf8=False):
        """gx_text_select on a host buffer: raw log text -> the text of the lines whose outcome `want` names, terminators included.
        Returns (selected text bytes, counts uint64[2K + 2], n_lines)."""
        raw = np.ascontiguousarray(np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else text, dtype=np.uint8)
        ptr = raw.ctypes.data if raw.size else None
        out = np.zeros(max(1, raw.size), np.uint8)   # (one pass: the selected text is no larger than the text)
        size, counts, n_lines = self.text_select_device(ptr, raw.size, want, out.ctypes.data, raw.size, device_pointers=False, utf8=utf8)
        return out[:size].tobytes(), counts, n_lines

    def text_select_device(self, text_ptr, size, want, out_ptr, out_cap, stream=None, device_pointers=True, utf8=False):
        """gx_text_select on device buffers (ints); out_ptr=None only asks for the sizes.  utf8: the text is UTF-8 and outcomes are those
        of the decoded Strings.  Returns (selected bytes, counts, n_lines)."""
        mask = self.want_mask(want)
        counts = np.zeros(2 * self.num_extractions + 2, np.uint64)
        o = N.gx_batch_opts()
        o.struct_size = C.sizeof(N.gx_batch_opts)
        o.device_pointers = 1 if device_pointers else 0
        o.stream = stream
        o.utf8 = 1 if utf8 else 0
        out_size, nl = C.c_uint64(0), C.c_uint64(0)
        _check(N.lib().gx_text_select(self._h.ptr, text_ptr, size, mask.ctypes.data, out_ptr, out_cap, C.byref(out_size), counts.ctypes.data,
                                      C.byref(nl), C.byref(o)))
        return out_size.value, counts, nl.value

    def results(self, data, offsets, match_id, caps, safe=False, utf8=None):
        """Materialise ExtractionResult objects (or None) for a finished batch.  utf8: what extract_batch was given -- "bytes":
        the lines are UTF-8 and the offsets index their bytes; "units": they index the decoded Strings' UTF-16 code units."""
        out = []
        raw = bytes(np.ascontiguousarray(data, dtype=np.uint8))
        mode = _utf8_mode(utf8)
        for i in range(len(match_id)):
            chunk = raw[int(offsets[i]):int(offsets[i + 1])]
            if mode == 0:
                out.append(self._materialise(chunk.decode("latin-1"), int(match_id[i]), caps[i], safe))
                continue
            line = chunk.decode("utf-8", "replace")
            if mode == 2:
                units = np.frombuffer(line.encode("utf-16-le", "surrogatepass"), dtype=np.uint16)
                out.append(self._materialise(line, int(match_id[i]), caps[i], safe, units=units))
            else:
                r = self._materialise(_ByteSlices(chunk), int(match_id[i]), caps[i], safe)
                if r is not None:
                    r._input = line
                out.append(r)
        return out


NUMBER_KINDS = ("long", "decimal", "iso8601", "clf")


def parse_number(kind, scale, text):
    """gx_parse_number: text (str, or bytes) as a number under the format (kind, scale) -- the rule the device applies to a captured
    value (set_number_format) -- or None when it is no number.  parse_number("iso8601", 3, "2026-01-03T00:00:00Z") is a term's
    number for a group read as epoch milliseconds."""
    if kind not in NUMBER_KINDS:
        raise ValueError("kind: long, decimal, iso8601 or clf")
    f = N.gx_number_format(NUMBER_KINDS.index(kind), int(scale))
    if isinstance(text, str):
        units = np.frombuffer(text.encode("utf-16-le"), dtype=np.uint16).copy()
    else:
        units = np.frombuffer(bytes(text), dtype=np.uint8).copy()
    value, is_number = C.c_int64(0), C.c_int32(0)
    _check(N.lib().gx_parse_number(C.byref(f), units.ctypes.data if units.size else None, units.size, 1 if units.dtype == np.uint16 else 0,
                                   C.byref(value), C.byref(is_number)))
    return int(value.value) if is_number.value else None


class _ByteSlices:
    """A UTF-8 line whose slices (by byte offsets) come back as decoded text."""

    def __init__(self, raw):
        self._raw = raw

    def __getitem__(self, s):
        return self._raw[s].decode("utf-8", "replace")


def _utf8_mode(utf8):
    """None / 0 / False -> 0; "bytes" / 1 / True -> 1; "units" / 2 -> 2 (gx_batch_opts.utf8)."""
    modes = {None: 0, 0: 0, "bytes": 1, 1: 1, "units": 2, 2: 2}
    if utf8 not in modes:
        raise ValueError('utf8: None, "bytes" or "units"')
    return modes[utf8]


def utf8_to_utf16(data, offsets):
    """gx_utf8_to_utf16 on host buffers: the UTF-8 lines of a CSR batch -> (units uint16[total], unit_offsets[n+1] of the
    offsets' dtype): the code units of the Strings Java would see, directly a utf16 batch for extract_batch."""
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets)
    if offsets.dtype not in (np.uint32, np.uint64):
        raise TypeError("offsets must be uint32 or uint64")
    n = len(offsets) - 1
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.offsets64 = 1 if offsets.dtype == np.uint64 else 0
    total = C.c_uint64(0)
    ptr = data.ctypes.data if data.size else None
    _check(N.lib().gx_utf8_to_utf16(ptr, offsets.ctypes.data, n, None, 0, None, C.byref(total), C.byref(o)))
    units = np.zeros(max(1, total.value), np.uint16)
    unit_offsets = np.zeros(n + 1, offsets.dtype)
    _check(N.lib().gx_utf8_to_utf16(ptr, offsets.ctypes.data, n, units.ctypes.data, total.value, unit_offsets.ctypes.data, C.byref(total), C.byref(o)))
    return units[:total.value], unit_offsets


def utf8_to_utf16_device(data_ptr, offsets_ptr, n, units_ptr, units_cap, unit_offsets_ptr, offsets64=False, stream=None):
    """gx_utf8_to_utf16 on device buffers (ints); units_ptr=None only asks for the size.  Returns the number of code units."""
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    o.offsets64 = 1 if offsets64 else 0
    o.stream = stream
    total = C.c_uint64(0)
    _check(N.lib().gx_utf8_to_utf16(data_ptr, offsets_ptr, n, units_ptr, units_cap, unit_offsets_ptr, C.byref(total), C.byref(o)))
    return total.value


def extract_batch_multi(gorps, data, offsets, match_only=False, strip_eol=False, compact=False):
    """gx_extract_batch_multi: one host CSR batch sharded by bytes over several Gorp objects (one per device, built
    from the same definition).  Returns what Gorp.extract_batch returns."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets)
    n = len(offsets) - 1
    G = gorps[0].max_groups
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.offsets64 = 1 if offsets.dtype == np.uint64 else 0
    o.match_only = 1 if match_only else 0
    o.strip_eol = 1 if strip_eol else 0
    hs = (C.c_void_p * len(gorps))(*[g._h.ptr for g in gorps])
    if compact and not match_only:
        rows = np.zeros((n, 1 + 2 * G), np.uint8 if int(compact) == 2 else np.uint16)
        over = C.c_uint64(0)
        o.compact_results = int(compact)
        o.overflow = C.cast(C.pointer(over), C.c_void_p)
        _check(N.lib().gx_extract_batch_multi(hs, len(gorps), data.ctypes.data if data.size else None, offsets.ctypes.data, n, None,
                                              rows.ctypes.data, C.byref(o)))
        return rows, over.value
    mid = np.zeros(n, np.int32)
    caps = np.full((n, 2 * G), -1, np.int32)
    _check(N.lib().gx_extract_batch_multi(hs, len(gorps), data.ctypes.data if data.size else None, offsets.ctypes.data, n, mid.ctypes.data,
                                          caps.ctypes.data if caps.size else None, C.byref(o)))
    return mid, caps


def unpack_rows(rows):
    """Compact rows uint16[n, 1 + slots] (or the u8 rows of compact=2) -> (match_id int32[n], caps int32[n, slots]) on the
    host (numpy)."""
    rows = np.asarray(rows)
    if rows.dtype in (np.uint8, np.int8):
        rows = rows.view(np.uint8)
        mid = rows[:, 0].astype(np.int8).astype(np.int32)
        caps = rows[:, 1:].astype(np.int32)
        caps[caps == 0xFF] = -1
        return mid, caps
    rows = rows.view(np.uint16) if rows.dtype == np.int16 else np.asarray(rows, dtype=np.uint16)
    mid = rows[:, 0].astype(np.int16).astype(np.int32)
    caps = rows[:, 1:].astype(np.int32)
    caps[caps == 0xFFFF] = -1
    return mid, caps


def extract_batch_multi_device(shards, match_only=False, strip_eol=False, compact=False, line_bytes_hint=0, max_line_bytes=0, no_sync=False,
                               offsets64=False):
    """gx_extract_batch_multi_device: device-resident CSR batches, one per Gorp object (= per device), in one call.
    shards: list of (gorp, data_ptr, offsets_ptr, n, match_id_ptr, caps_ptr, overflow_ptr or None, stream or None)."""
    arr = (N.gx_device_shard * len(shards))()
    for a, (g, d, o_, n, m, c, ov, st) in zip(arr, shards):
        a.handle, a.bytes, a.offsets, a.n, a.match_id, a.caps, a.overflow, a.stream = g._h.ptr, d, o_, n, m, c, ov, st
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.match_only = 1 if match_only else 0
    o.strip_eol = 1 if strip_eol else 0
    o.compact_results = int(compact)
    o.line_bytes_hint = int(line_bytes_hint)
    o.max_line_bytes = int(max_line_bytes)
    o.no_sync = 1 if no_sync else 0
    o.offsets64 = 1 if offsets64 else 0
    _check(N.lib().gx_extract_batch_multi_device(arr, len(shards), C.byref(o)))


def create_on_devices(gorp, devices, flags=0):
    """gx_create_on_devices: `gorp`'s tables (its blob) on every device of `devices` -- the first handle from the blob, the others'
    device images copied from the first one's device (over xGMI between peers).  Returns one Gorp per device, same extractions."""
    blob = np.ascontiguousarray(gorp.blob())
    devs = (C.c_int32 * len(devices))(*[int(d) for d in devices])
    hs = (C.c_void_p * len(devices))()
    _check(N.lib().gx_create_on_devices(blob.ctypes.data, len(blob), devs, len(devices), flags | DEFAULT_CREATE_FLAGS, hs))
    return [Gorp(_Handle(C.c_void_p(h)), gorp._extractions) for h in hs]


def gather_rows(shards, row_bytes, dst_device, dst_ptr, no_sync=False):
    """gx_gather_rows: shards = list of (gorp, rows_ptr, n, stream or None); the rows of all shards onto `dst_device` at dst_ptr,
    in shard order, each shard's copy behind its kernel on a copy stream of the shard's device."""
    arr = (N.gx_rows_shard * len(shards))()
    for a, (g, r, n, st) in zip(arr, shards):
        a.handle, a.rows, a.n, a.stream = g._h.ptr, r, n, st
    _check(N.lib().gx_gather_rows(arr, len(shards), int(row_bytes), int(dst_device), dst_ptr, 1 if no_sync else 0))


def gather_wait(gorps):
    hs = (C.c_void_p * len(gorps))(*[g._h.ptr for g in gorps])
    _check(N.lib().gx_gather_wait(hs, len(gorps)))


def split_lines(data, cap_lines=None, offsets_dtype=np.uint32, want_flags=False):
    """gx_split_lines on a host buffer: raw bytes -> (offsets[n+1], flags[n] or None) with readLine() line
    boundaries; every line keeps its terminator (pass strip_eol=True to extract_batch)."""
    data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
    if cap_lines is None:
        cap_lines = int(data.size) + 1
    offsets = np.zeros(cap_lines + 1, offsets_dtype)
    flags = np.zeros(cap_lines, np.uint8) if want_flags else None
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.offsets64 = 1 if np.dtype(offsets_dtype) == np.uint64 else 0
    n = C.c_uint64(0)
    _check(N.lib().gx_split_lines(data.ctypes.data if data.size else None, data.size, offsets.ctypes.data, cap_lines, C.byref(n),
                                  flags.ctypes.data if want_flags and cap_lines else None, C.byref(o)))
    return offsets[:n.value + 1], (flags[:n.value] if want_flags else None)


def pack_results_device(match_id_ptr, caps_ptr, n, slots, packed_ptr, stream=None):
    """gx_pack_results: int32 rows -> [int16 id, uint16 offsets] rows on the device; returns the overflow count."""
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    o.stream = stream
    over = C.c_uint64(0)
    _check(N.lib().gx_pack_results(match_id_ptr, caps_ptr, n, slots, packed_ptr, C.byref(over), C.byref(o)))
    return over.value


def unpack_results_device(packed_ptr, n, slots, match_id_ptr, caps_ptr, stream=None, narrow=False):
    """gx_unpack_results (u16 rows) / gx_unpack_results8 (narrow=True: the u8 rows of compact=2) on the device."""
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    o.stream = stream
    fn = N.lib().gx_unpack_results8 if narrow else N.lib().gx_unpack_results
    _check(fn(packed_ptr, n, slots, match_id_ptr, caps_ptr, C.byref(o)))


def split_lines_device(data_ptr, size, offsets_ptr, cap_lines, flags_ptr=None, offsets64=False, stream=None, want_max=False):
    """gx_split_lines on device buffers (ints, e.g. torch data_ptr()); returns the number of lines -- with want_max
    (gx_split_lines_max) the pair (lines, length of the longest line with its terminator)."""
    o = N.gx_batch_opts()
    o.struct_size = C.sizeof(N.gx_batch_opts)
    o.device_pointers = 1
    o.offsets64 = 1 if offsets64 else 0
    o.stream = stream
    n = C.c_uint64(0)
    if want_max:
        m = C.c_uint64(0)
        _check(N.lib().gx_split_lines_max(data_ptr, size, offsets_ptr, cap_lines, C.byref(n), flags_ptr, C.byref(m), C.byref(o)))
        return n.value, m.value
    _check(N.lib().gx_split_lines(data_ptr, size, offsets_ptr, cap_lines, C.byref(n), flags_ptr, C.byref(o)))
    return n.value


def lines_to_csr(lines, offsets_dtype=np.uint32):
    """Pack str/bytes lines into the CSR byte buffer gx_extract_batch consumes (Latin-1)."""
    bs = [ln if isinstance(ln, (bytes, bytearray)) else ln.encode("latin-1") for ln in lines]
    offsets = np.zeros(len(bs) + 1, dtype=offsets_dtype)
    if bs:
        offsets[1:] = np.cumsum([len(b) for b in bs])
    data = np.frombuffer(b"".join(bs), dtype=np.uint8) if bs else np.zeros(0, np.uint8)
    return data, offsets


# ---------------------------------------------------------------------------
# DefinitionReader (core/DefinitionReader.java) -- the definition language, parsed natively (gx_dsl.cpp)
# ---------------------------------------------------------------------------
def _definition_json(text, source_ref, stage):
    import json
    L = N.lib()
    raw = _c_text(text)
    cap = 64 * len(raw) + 4096
    n = C.c_size_t(0)
    buf = C.create_string_buffer(cap)
    rc = L.gx_definition_to_json(raw, source_ref.encode("utf-8"), stage.encode("ascii"), buf, cap, C.byref(n))
    if rc == N.GX_E_ARG and n.value + 1 > cap:
        cap = n.value + 1
        buf = C.create_string_buffer(cap)
        rc = L.gx_definition_to_json(raw, source_ref.encode("utf-8"), stage.encode("ascii"), buf, cap, C.byref(n))
    if rc == N.GX_E_DEFINITION:
        raise DefinitionParseException(rc, N.last_error())
    _check(rc)
    return json.loads(buf.raw[:n.value].decode("utf-8"))


class DefinitionReader:
    """core/DefinitionReader.java: reads an extraction definition and builds a Gorp."""

    def __init__(self, text, source_ref):
        self._text = text
        self._source_ref = source_ref

    @staticmethod
    def reader(source):
        """`source`: definition text, or a path-like object / open file (DefinitionReader.reader(File|String))."""
        import os
        if hasattr(source, "read"):
            return DefinitionReader(source.read(), "<input stream>")
        if isinstance(source, os.PathLike):
            path = os.fspath(source)
            with open(path, encoding="utf-8") as f:
                return DefinitionReader(f.read(), "file '%s'" % os.path.abspath(path))
        return DefinitionReader(source, "<input string>")

    def readUncooked(self):
        """Tokenised but unresolved definitions (dict view of UncookedDefinitions)."""
        return _definition_json(self._text, self._source_ref, "uncooked")

    def resolveTemplates(self):
        """Resolved patterns and templates (dict view of CookedDefinitions after resolveTemplates)."""
        return _definition_json(self._text, self._source_ref, "cooked")

    def flatten(self):
        """List of FlattenedExtraction (CookedDefinitions.getExtractions())."""
        d = _definition_json(self._text, self._source_ref, "flattened")
        return [FlattenedExtraction(x["name"], x["pieces"], x["append"]) for x in d["extractions"]], d

    def read(self, host_only=False, flags=0):
        """DefinitionReader.read() (core/DefinitionReader.java:74-84): the native front-end parses, resolves and
        compiles the definition in one call (gx_create_from_definition)."""
        fl, d = self.flatten()
        cooked = [CookedExtraction(i, x["name"], x["jdk_rx"], x["extractor_names"], x["append"])
                  for i, x in enumerate(d["extractions"])]
        hp = C.c_void_p()
        rc = N.lib().gx_create_from_definition(_c_text(self._text), self._source_ref.encode("utf-8"),
                                               flags | DEFAULT_CREATE_FLAGS | (N.GX_CREATE_HOST_ONLY if host_only else 0), C.byref(hp))
        if rc in (N.GX_E_DEFINITION, N.GX_E_REGEX_SYNTAX, N.GX_E_UNSUPPORTED_CONSTRUCT, N.GX_E_LIMIT):
            raise DefinitionParseException(rc, N.last_error())
        _check(rc)
        g = Gorp(_Handle(hp), cooked)
        g._meta_sent = True  # the native front-end kept the names itself
        return g
