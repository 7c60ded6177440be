/*
 * gorp_hip.h -- C ABI of libgorp_hip.so: the MI355X (gfx950) implementation of
 * Gorp's combined-DFA match-and-extract hot path.
 *
 * Every entry point cites the reference interface it replaces
 * (core/ = gorp-core/src/main/java/com/salesforce/gorp/ in salesforce/gorp).
 * Plain pointers and sizes only; no exceptions cross this boundary; no torch
 * types.  INTEGRATION.md shows the JNI stub that binds these from Java.
 *
 * Per-line results are DATA, never call failures:
 *   match_id >= 0      index of the first-declared matching extraction
 *                      (matchIndexes[0], core/Gorp.java:166)
 *   match_id == -1     no extraction matches -> Gorp.extract returns null
 *                      (core/Gorp.java:162-164)
 *   match_id == -2-k   the DFA chose extraction k but its capture regex
 *                      rejected the line -> ExtractionException
 *                      (core/Gorp.java:173-177); extractSafe returns null
 *                      for exactly these lines (core/Gorp.java:178-185)
 * Captures: for g < gx_num_groups(h, match_id): caps[2g], caps[2g+1] are the
 * begin/end offsets of Matcher.group(g+1) in code units from the start of the
 * line (core/jdkre/JDKRegexpCookedExtraction.java:51-59); -1,-1 when group()
 * would return null.  Slots beyond the matched extraction's group count are -1.
 */
#ifndef GORP_HIP_H
#define GORP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gx_handle gx_handle;

/* Error classes (return values; 0 = OK).  Reference conventions they stand for:
 * invalid regex -> IllegalArgumentException "Invalid regexp, ..." wrapped in
 * DefinitionParseException (core/autom/PolyMatcher.java:79-81, core/Gorp.java:84-90). */
enum {
    GX_OK = 0,
    GX_E_REGEX_SYNTAX = 1,         /* a pattern does not parse in its dialect */
    GX_E_UNSUPPORTED_CONSTRUCT = 2,/* valid java.util.regex, outside Gorp's documented subset (README.md:209-224) */
    GX_E_DEVICE = 3,               /* no gfx950 device / HIP runtime failure */
    GX_E_ARG = 4,                  /* bad argument */
    GX_E_NOMEM = 5,
    GX_E_LIMIT = 6,                /* automaton exceeds a compile-time limit */
    GX_E_DEFINITION = 7            /* definition text rejected: DefinitionParseException (core/DefinitionParseException.java) */
};

/* gx_create flags */
#define GX_CREATE_HOST_ONLY 1u     /* compile tables only; do not touch the GPU (used to build the
                                      blob that is broadcast to other ranks, and by CPU-only checks) */
/* Kernel choice, for measurements and tests; results never depend on it.  By default the automaton rows live in
 * LDS when they fit, else in global memory (L2), and the capture automata are fused with the match automaton
 * when that product stays within the size limits. */
#define GX_CREATE_TIER_L2   2u     /* keep the automaton rows in global memory even when they would fit LDS */
#define GX_CREATE_NO_TILES  4u     /* per-line kernel only */
#define GX_CREATE_NO_FUSED  8u     /* two passes: match automaton, then the winning extraction's capture automaton */
#define GX_CREATE_TIER_RECORDS 16u /* sparse range records in LDS even when the dense rows would fit (the default when they do
                                      not: BASELINE configs[2], 64 extractions) */
#define GX_CREATE_TIER_RECORDS_GLOBAL 32u /* sparse range records in global memory (L1 / L2 resident) */
#define GX_CREATE_TIER_HOP  64u    /* build the hop tier's tables (run + literal chain per state, hot states in LDS, dense rows in
                                      global memory as the backstop) even when the dense rows fit LDS; the default for capture
                                      batches when they do not */
#define GX_CREATE_PROGRAMS  256u   /* every extraction that can be run as a program (at most 256 character classes, at most 32 groups)
                                      keeps its program and no capture automaton is built for it: the per-line kernel runs it as it
                                      does an extraction whose automaton would be too large (gx_stat(h, 27)).  Any other extraction keeps
                                      its automaton.  Without it the size of that automaton alone decides.  gx_create_from_blob and
                                      gx_create_on_devices ignore it: the blob says what it holds. */

#define GX_CREATE_RESIDENT_ONE 128u /* gx_extract_one_utf16 without a kernel launch per call: while such calls keep coming the handle keeps
                                      one wave resident on the device (tables in LDS) that takes the line out of pinned host memory and
                                      puts the answer back -- a few stores and a spin on the host's side, about 5 us instead of 22.  The wave
                                      leaves by itself when no call has come for 0.3 ms (the next call starts it again, at the price of
                                      a launch) and after 20 ms in any case, so a device-wide synchronisation elsewhere in the process
                                      waits milliseconds at most.  For definitions whose dense rows fit LDS and Latin-1 lines of up to
                                      1 016 characters; every other call takes the usual path.  Off by default: it holds LDS and a
                                      wave slot of one CU while it is resident. */

/* Replaces Gorp.construct's per-extraction back half (core/Gorp.java:58-92):
 * PolyMatcher.create(automatonInputs) (core/autom/PolyMatcher.java:64-84 ->
 * Automata.construct, core/autom/Automata.java:57-124) and
 * ExtractionCooker.cook -> Pattern.compile (core/jdkre/JDKRegexpExtractionCooker.java:20-26).
 * Inputs are exactly the two regex strings per extraction that
 * Gorp._buildExtractor emits (core/Gorp.java:94-129), UTF-8 encoded.
 * jdk_rx may be NULL: matcher only (PolyMatcher.create), no captures.
 * The group count of extraction k is read from jdk_rx[k] itself
 * (Matcher.groupCount()). */
int gx_create_from_patterns(const char* const* automaton_rx, const char* const* jdk_rx,
                            int32_t n, uint32_t flags, gx_handle** out);

/* Packed, relocatable table blob (the RCCL broadcast payload): rank 0 compiles,
 * every rank calls gx_create_from_blob.  gx_blob_size returns the byte count;
 * gx_blob_copy writes it to dst. */
size_t gx_blob_size(const gx_handle* h);
int gx_blob_copy(const gx_handle* h, void* dst, size_t cap);
int gx_create_from_blob(const void* blob, size_t size, uint32_t flags, gx_handle** out);

/* Frees host and device tables.  (Java GC in the reference.) */
void gx_destroy(gx_handle* h);

/* Introspection (Automata.size(), core/autom/Automata.java:129-131; Matcher.groupCount()). */
int32_t gx_num_extractions(const gx_handle* h);
int32_t gx_num_groups(const gx_handle* h, int32_t k);
int32_t gx_max_groups(const gx_handle* h);
/* table statistics: 0 = match-DFA states, 1 = char classes, 2 = capture-automaton states (sum),
 * 3 = capture registers (max over extractions), 4 = blob bytes, 5 = LDS bytes the batch kernel stages,
 * 6 = waves per workgroup of the batch kernel, 7 = table tier of the batch kernel (1 = automaton rows in LDS,
 * 2 = rows in global memory / L2, 3 = sparse range records in LDS, 4 = range records in global memory, 0 = per-line
 * generic kernel), 9 = the same for match-only batches (a large definition keeps a second, smaller table image for them),
 * 8 = 1 when the handle has capture regexps, 10 / 11 = waves per workgroup of the lane kernel (captures with compact rows /
 * match only; 0 where it does not apply), 12 = bytes of the batch kernels' table image, 13 = bytes of a wave's register block;
 * the hop tier (run + chain records for capture batches of definitions whose dense rows do not fit LDS): 14 = its states
 * (0: the handle has no hop tables), 15 / 21 = states whose records are in LDS under the tile kernel / the hop slice kernel,
 * 16 = states that well-formed lines reach, 17 = states that have a chain, 18 / 19 = waves per workgroup of the tile kernel on
 * these tables / of the hop slice kernel, 20 = branching states whose dense row is in LDS too, 22 / 23 = states / states with
 * their records in LDS of the second hop image, built from the match automaton alone for match-only batches;
 * 24 = batches that broke their gx_batch_opts.max_line_bytes promise, as far as calls have made good for them or reported them
 * (every such batch is counted once; it never moves while all promises hold); 25 = the kernel the most recent batch ran on
 * (a GX_KERNEL_* value; 0: none yet); 31 / 32 = for that most recent batch launch, the longest line (code units in memory,
 * terminator included) for which a max_line_bytes promise drops the follow-up launch, and the figure the kernel's own rule about
 * the lines it leaves is stated in -- a wave's staging area in bytes for the tile kernels (a line stays when its units + the 0..15
 * its address adds + 48 are within it), the longest line without its terminator for the lane and hop slice kernels (0 / 0: a
 * kernel that leaves no line; read-only, for tests that must know where that edge lies); 26 = why capture batches have no hop tables (0: they have; 1: no fused automaton or no
 * capture regexps; 2: a step with capture programs other than one "register := position" -- groups that may match the empty string
 * write two registers in one step; 3: beyond a limit of the tier; 4: not built -- the dense rows fit LDS, or the caller named another
 * tier; 5: the tables leave no room for a wave); 27 = extractions whose capture automaton would be too large ahead of time and
 * whose regexp is therefore RUN as a program, thread lists in priority order (exact, linear in line x program; such a definition's
 * batches go through the per-line kernel); 28 = times the resident one-line wave was started (GX_CREATE_RESIDENT_ONE; -1: the
 * handle has none); 33 / 34 = for the most recent gx_batch_opts.utf8 batch (gx_extract_batch, gx_text_to_jsonl, gx_text_select): the lines that
 * held a byte >= 0x80 and were walked again as Strings, and the UTF-16 code units made for them;
 * 35 = the workgroups of 256 lanes a per-line launch of this handle is kept within, every lane that may run a program having its own
 * thread lists (-1: the handle has no extraction that runs as a program);
 * what the batch kernels' table image was built from (read-only, for tests that must know how near an image is to a limit of its
 * format): 36 / 37 = the range records of the batch image / of the image match-only batches walk (0: dense rows, or no image),
 * 38 = the automaton rows (states) the batch image covers, 39 = 1 when its capture side is the fused automaton (0: one capture
 * automaton per extraction -- the two-pass layout --, no capture regexps, or no image) */
int64_t gx_stat(const gx_handle* h, int32_t which);

typedef struct gx_batch_opts {
    uint32_t struct_size;      /* = sizeof(gx_batch_opts) */
    uint32_t device_pointers;  /* 1: bytes/offsets/match_id/caps are device pointers on the handle's device */
    uint32_t offsets64;        /* 1: offsets are uint64_t[n+1] instead of uint32_t[n+1] */
    uint32_t match_only;       /* 1: PolyMatcher.match only; caps may be NULL */
    void*    stream;           /* hipStream_t to launch on (NULL = the null stream) */
    uint32_t no_sync;          /* 1 (device pointers only): return after enqueueing */
    uint32_t line_bytes_hint;  /* typical line length in bytes; sizes the per-wave LDS staging area of the batch kernel.
                                  A wrong hint costs speed, never correctness.  0: the batch's mean line length -- read
                                  from the offsets (a small synchronous copy), or with no_sync the mean of the previous
                                  no_sync batch of this handle (200 until one has completed) */
    uint32_t strip_eol;        /* 1: every line carries its terminator ("\n", "\r\n" or "\r", as produced by
                                  gx_split_lines); it is not part of the String the reference would see, so
                                  it is ignored and capture offsets stay relative to the start of the line */
    uint32_t utf8_passthrough; /* gx_results_to_jsonl only.  0: line bytes are Latin-1 code units (the batch path's input
                                  model) and bytes >= 0x80 leave as two-byte UTF-8; 1: copy them unchanged (the
                                  input was UTF-8 all along and the patterns only look at its ASCII structure) */
    uint32_t utf16;            /* gx_extract_batch only.  1: `bytes` holds UTF-16 code units (uint16_t, host byte order), exactly
                                  the chars of the Java Strings, and offsets count code units.  On dense rows in LDS and on
                                  hop tables (gx_stat(h, 7) == 1 or gx_stat(h, 14) > 0, kernel AUTO) the batch kernels read
                                  the units themselves: no copy, no synchronisation, no_sync means what it says.  On the
                                  other tables, or with a kernel named in `kernel`, the units' low bytes go through the byte
                                  kernels as a narrowed copy, sized by a read of the offsets' two ends ON THE HOST: such a
                                  batch cannot be no_sync and is refused with GX_E_ARG when it asks for it (round 5; until
                                  then the flag was silently not honoured there).  Either way only the lines that hold a
                                  unit above 0xFF are walked again, per line, on the code units.  (With compact rows, an
                                  offset that does not fit is counted once per walk: such a line is walked twice.) */
    uint32_t kernel;           /* gx_extract_batch only: GX_KERNEL_AUTO (0) or one of the kernels below, for measurements and
                                  tests; results never depend on it.  (New fields are only ever appended: a caller compiled
                                  against an older, shorter layout passes its own struct_size and keeps working.) */
    uint32_t compact_results;  /* gx_extract_batch only.  1: results leave as compact rows -- `caps` points to
                                  uint16_t[n * (1 + 2*gx_max_groups(h))], per line the match id as int16 followed by the capture
                                  offsets, 0xFFFF = unset (the layout of gx_pack_results); match_id may be NULL.  Half the
                                  result bytes of the dense format; what the gather between GPUs sends.  An offset above
                                  65534 does not fit: it is stored as 65534 and counted in *overflow (take such a batch again
                                  in the dense format).  2: u8 rows instead -- `caps` points to uint8_t[n * (1 + 2*gx_max_groups(h))],
                                  the match id as int8 and the offsets with 0xFF = unset: a quarter of the dense bytes, for
                                  batches whose lines are shorter than 255 bytes (log lines mostly are) and definitions of at
                                  most 126 extractions (GX_E_ARG beyond).  An offset above 254 is stored as 254 and counted in
                                  *overflow.  Ignored with match_only. */
    uint32_t uneven_lines;     /* gx_extract_batch only.  Lines run in lock step in groups of 64: a group takes as long as its longest
                                  line.  2: the lines differ much in length -- the kernels then group lines of similar length where
                                  they can (results are the same); 1: they do not; 0: the library looks itself where it can see
                                  the offsets without waiting (host pointers; device pointers without no_sync and without a hint),
                                  and assumes 1 elsewhere.  Batches with a mean length above 255 bytes are taken as uneven. */
    void*    overflow;         /* with compact_results: uint64_t counter that the call ADDS to (the caller zeroes it); a device
                                  pointer with device_pointers, else a host pointer.  NULL: not counted.  Every clipped offset
                                  is counted once -- with one known exception: a utf16 batch that goes through the narrowed copy
                                  of its code units (tables other than dense rows in LDS or hop tables, or a kernel named in
                                  `kernel`) counts the clipped offsets of a line that holds a unit above 0xFF twice (the byte
                                  kernel's pass over the low bytes, then the per-line walk that writes the row); the rows are
                                  right.  A utf8 batch has the same exception for its lines that are not ASCII (see utf8). */
    uint32_t max_line_bytes;   /* gx_extract_batch with device_pointers.  The caller's PROMISE: no line of the batch -- offsets[i+1] -
                                  offsets[i], terminator included -- is longer than this many code units (0: no promise).
                                  gx_split_lines_max reports it for free; a log shipper knows its own cap.  Without it every batch
                                  kernel is followed by a second, nearly empty launch that takes the lines the batch kernel cannot
                                  stage (longer than a wave's staging area: about 64 x line_bytes_hint bytes; 65 535 for the lane
                                  and hop slice kernels); with it, and when it is within what the chosen kernel takes, that launch
                                  is dropped (1-2 % of a 10 M-line batch).  A promise that does not hold is detected, never
                                  silently wrong: without no_sync the call sees it when it synchronises, runs the follow-up then and
                                  returns the right results (gx_extract_batch_multi_device without no_sync does the same for every
                                  shard: rows and *overflow as if no promise had been made); with no_sync the longer line's result
                                  row is left UNWRITTEN and its offsets uncounted, and a later call on the same stream fails with
                                  GX_E_ARG -- the next gx_extract_batch (or shard) submitted once that batch has run, which is then
                                  not launched, or the first call that waits for a batch of its own behind it, whose own rows are
                                  complete all the same; at the latest the first call made after the stream has drained.  One
                                  error stands for every batch of the stream that broke its promise since the last one; each is
                                  counted in gx_stat(h, 24), once.  The streams beyond a handle's 31st share one flag word: a break
                                  on one of them is reported to whichever of them calls next, and a synchronous call of one
                                  whose word another's later launch has overwritten is not made good but reported like a
                                  no_sync batch (by an error whose text then wrongly calls some batch complete: check rows). */
    uint32_t utf8;             /* gx_extract_batch, gx_text_to_jsonl, gx_text_select (1 only).  The lines are UTF-8 and are read as the Strings
                                  Java would see (new InputStreamReader(in, "UTF-8")): 0: off -- a byte is one Latin-1 code unit;
                                  1: capture offsets are BYTES of the line as it lies in memory -- what a caller that holds bytes
                                  slices with, and what gx_results_to_jsonl with utf8_passthrough = 1 needs; 2: capture offsets are
                                  UTF-16 CODE UNITS of the decoded String, Matcher.start() / end().  Ill-formed input decodes to
                                  U+FFFD per maximal subpart (Unicode 3.9; what CPython's "replace" handler does); a JDK may differ
                                  in the NUMBER of U+FFFD for some ill-formed input (encoded surrogates ED A0 80, for instance),
                                  never for well-formed input; no BOM handling (Java keeps U+FEFF too).  A sequence never
                                  continues across a line's end.  The byte batch kernel runs as ever -- its rows are right for every
                                  ASCII-only line -- and the lines that hold a byte >= 0x80 are transcoded and walked again, per
                                  line, on their code units (gx_stat(h, 33) / (h, 34): how many lines, how many units).  That
                                  fix-up reads two numbers on the host to size its memory: with no_sync it is refused (GX_E_ARG),
                                  as with utf16, with gx_match_batch and in gx_extract_batch_multi / _multi_device.  Host pointers
                                  stage the whole batch to the device and back (no chunk pipeline).  With compact rows, the clipped
                                  offsets of a line that is walked again are counted more than once in *overflow (the byte pass,
                                  the walk on units, and utf8 = 1's step back to bytes); the rows are right.  gx_text_to_jsonl
                                  with utf8 writes with utf8_passthrough semantics: the line's bytes leave as they are, ill-formed
                                  ones included (they are not repaired).  (This field lies in what was tail padding: struct_size
                                  of the layout that ended with max_line_bytes reads as utf8 = 0.) */
    void*    utf8_line_flags;  /* with utf8, optional: uint8_t[n], != 0 for every line that holds a byte >= 0x80 -- the line_flags of
                                  gx_split_lines for exactly these lines (a device pointer with device_pointers).  Saves the sweep
                                  over the batch that finds them.  A line wrongly flagged 0 is read as Latin-1. */
} gx_batch_opts;

enum { GX_KERNEL_AUTO = 0, GX_KERNEL_TILES = 1, GX_KERNEL_SLICES = 2, GX_KERNEL_PER_LINE = 3, GX_KERNEL_LANES = 4,
       GX_KERNEL_HOPS = 5 /* the tile kernel on the hop tier's tables (where the handle has them: gx_stat(h, 14)) */,
       GX_KERNEL_HOP_SLICES = 6 /* the same tables under the slice kernel's staging: long and uneven lines */ };

/* Replaces the per-line loop "for each line: Gorp.extract(line)"
 * (core/Gorp.java:145-186 -> PolyMatcher.match core/autom/PolyMatcher.java:123-133
 *  -> JDKRegexpCookedExtraction.match core/jdkre/JDKRegexpCookedExtraction.java:36-59)
 * over a batch held as one CSR byte buffer: line i = bytes[offsets[i] .. offsets[i+1]),
 * each byte one Latin-1 code unit.  match_id[n]; caps[n * 2*gx_max_groups(h)] dense. */
int gx_extract_batch(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n,
                     int32_t* match_id, int32_t* caps, const gx_batch_opts* opts);

/* Line ingestion, the step before the path.  The reference has no counterpart: its callers pass
 * java.lang.Strings read from "a line-oriented input source" (README.md:26) -- BufferedReader.readLine(),
 * whose lines end at "\n", "\r" or "\r\n", the last line needing no terminator.  For a raw byte buffer this
 * writes offsets[0..n] with line i = bytes[offsets[i], offsets[i+1]) INCLUDING its terminator, ready for
 * gx_extract_batch with strip_eol = 1.  offsets holds cap_lines + 1 entries (uint32_t, or uint64_t with
 * opts->offsets64; a uint32_t buffer must be < 4 GiB).  line_flags (optional, cap_lines bytes) receives 1 for
 * every line containing a byte >= 0x80: such a line is Latin-1 only if the file is; for UTF-8 text hand the
 * flags to gx_extract_batch as gx_batch_opts.utf8_line_flags with gx_batch_opts.utf8 (or transcode with gx_utf8_to_utf16).  Runs on the GPU (three bandwidth-bound passes); with opts->device_pointers = 1
 * bytes / offsets / line_flags are device pointers (bytes 16-byte aligned) and *n_lines (host) is written
 * after a stream synchronisation.  GX_E_LIMIT when the buffer holds more than cap_lines lines (*n_lines is
 * still set, so the caller can retry with a larger offsets array). */
int gx_split_lines(const uint8_t* bytes, uint64_t size, void* offsets, uint64_t cap_lines, uint64_t* n_lines,
                   uint8_t* line_flags, const gx_batch_opts* opts);
/* The same, and *max_line_bytes (host, optional) receives the length of the longest line, terminator included: what
 * gx_batch_opts.max_line_bytes wants to hear (the pass that writes the offsets sees every line end anyway). */
int gx_split_lines_max(const uint8_t* bytes, uint64_t size, void* offsets, uint64_t cap_lines, uint64_t* n_lines,
                       uint8_t* line_flags, uint64_t* max_line_bytes, const gx_batch_opts* opts);

/* UTF-8 lines -> the UTF-16 code units of the Strings Java would see, EVERY line of a CSR batch (ASCII lines widened): what
 * new InputStreamReader(in, "UTF-8") does before the reference sees a line.  The decoding rule is gx_batch_opts.utf8's.  line i =
 * bytes[offsets[i] .. offsets[i+1]); nothing outside a line is looked at and nothing outside the batch is read.  units receives the
 * code units (host byte order), unit_offsets n + 1 entries of the input offsets' width (opts->offsets64), starting at 0: together
 * directly a gx_batch_opts.utf16 batch.  *n_units (host) is always set; units == NULL only asks for it; GX_E_LIMIT when units_cap
 * (in units) is too small -- nothing has been written -- or when uint32_t offsets cannot hold the total.  opts: device_pointers
 * (bytes / offsets / units / unit_offsets on the current device; else they are staged), stream, offsets64.  Three passes -- count,
 * scan, write -- with one synchronisation between scan and write.  No handle: one workspace per device, kept between calls (12 bytes
 * per line of the largest batch; gx_release_scratch gives it back). */
int gx_utf8_to_utf16(const uint8_t* bytes, const void* offsets, uint64_t n, uint16_t* units, uint64_t units_cap, void* unit_offsets,
                     uint64_t* n_units, const gx_batch_opts* opts);

/* Result materialisation, the step after the path: ExtractionResult.asMap(idAs)
 * (core/ExtractionResult.java:65-88) for every matched line of a finished batch, written as one JSON object per
 * line ("JSON Lines") the way Jackson serialises the LinkedHashMap: the id first when id_as != NULL, then
 * extractor name -> captured text in group order (null where Matcher.group() is null), then the extraction's
 * `append` entries (core/DefinitionReader.java:602-640); a key put twice keeps its first position and its last
 * value.  Lines with match_id < 0 produce no text.  bytes/offsets/match_id/caps are the arguments and results
 * of gx_extract_batch.  line_out_offsets (optional, n + 1 entries) receives where each line's text starts
 * (equal neighbours = no text).  *out_size receives the total; out == NULL only asks for the size; GX_E_LIMIT
 * when out_cap is too small.  With opts->device_pointers = 1 every buffer except out_size is a device pointer.
 * Needs the extraction names: a handle from gx_create_from_definition, or gx_set_extraction_meta first.
 * The call's device workspace (sizes, line offsets; for gx_text_to_jsonl also the lines' offsets, ids and capture rows) stays
 * allocated on the handle and is reused by later calls (it grows to what the largest batch asked for; gx_destroy frees it);
 * likewise the narrowed copy of a utf16 batch (a memory pool of the handle's own). */
int gx_results_to_jsonl(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, const int32_t* match_id,
                        const int32_t* caps, const char* id_as, uint8_t* out, uint64_t out_cap, uint64_t* out_size,
                        uint64_t* line_out_offsets, const gx_batch_opts* opts);

/* The three steps in one call, for whole files: raw text -> lines (gx_split_lines semantics) -> the match-and-extract
 * path (terminators ignored) -> JSON Lines (gx_results_to_jsonl semantics).  What the reference's caller writes as
 *     while ((line = reader.readLine()) != null) { r = gorp.extract(line); if (r != null) write(json(r.asMap(idAs))); }
 * (README.md:26,63-79), with extractSafe semantics for lines the capture regexp rejects (no text, counted in
 * *n_exceptions).  Intermediate buffers live and die on the device.  *n_lines / *n_matched / *n_exceptions (each
 * optional) receive the counts; *out_size the size of the text; out == NULL only asks for the size; GX_E_LIMIT when
 * out_cap is too small.  opts: device_pointers (text and out on the device), stream, utf8_passthrough, utf8 (1: the text is UTF-8 --
 * outcomes, counts and JSON values are those of the decoded Strings; implies utf8_passthrough).  Text of 4 GiB
 * and more must be split by the caller (at a line boundary). */
int gx_text_to_jsonl(gx_handle* h, const uint8_t* text, uint64_t size, const char* id_as, uint8_t* out, uint64_t out_cap,
                     uint64_t* out_size, uint64_t* n_lines, uint64_t* n_matched, uint64_t* n_exceptions, const gx_batch_opts* opts);

/* Outcomes of a finished batch, on the device.  The reference has no counterpart: its caller sees every line's outcome in its own
 * loop, "while ((line = readLine()) != null) { r = gorp.extract(line); ... }" (README.md:26,63-79) -- a null result is a line no
 * extraction matched and can be kept aside, an ExtractionException is a definition bug and the line can be logged, a result goes to
 * the sink of its extraction (the three outcomes: core/Gorp.java:159-186).  In bulk the outcomes are match ids in device memory;
 * these calls count them and pick lines by them without a copy to the host.  They are named through the OUTCOME INDEX over
 * K = gx_num_extractions(h):
 *     id in [0, K)   ->  id            matched extraction id
 *     id == -1       ->  K             no match
 *     id == -2-k     ->  K + 1 + k     exception of extraction k (0 <= k < K)
 *     anything else  ->  2K + 1        a row nobody wrote (a broken max_line_bytes promise): counted, never selected
 * ids is read in the format opts->compact_results names: 0: int32_t match_id[n]; 1 / 2: the u16 / u8 result rows of
 * 1 + 2 * gx_max_groups(h) units, whose first unit is the id.
 *
 * gx_count_outcomes: counts[2K + 2] (host) receives the number of lines per outcome index.  opts: device_pointers (ids on the
 * device; else it is staged), stream, compact_results.  Synchronises the stream to deliver the counts. */
int gx_count_outcomes(gx_handle* h, const void* ids, uint64_t n, uint64_t* counts, const gx_batch_opts* opts);

/* gx_select_lines: the lines whose outcome index x has want[x] != 0 (want: uint8_t[2K + 1] on the host), in input order.  The
 * batch is bytes / offsets / n as for gx_extract_batch (opts->offsets64, opts->utf16: two-byte code units, offsets in units), ids as
 * above, caps the dense capture rows (compact_results 0 only, and only needed for out_caps).  Outputs, each optional (NULL):
 *   out_index    uint32_t[cap_lines]: the kept lines' numbers in the input (n of 2^32 and more: GX_E_LIMIT);
 *   out_bytes    out_bytes_cap bytes, and out_offsets, cap_lines + 1 entries of the input offsets' width: a new CSR batch -- every
 *                kept line copied exactly as bytes[offsets[i] .. offsets[i+1]), terminator included if it had one; out_offsets
 *                starts at 0, counts code units, and has *n_selected + 1 entries.  Directly an input of gx_extract_batch and
 *                gx_results_to_jsonl;
 *   out_ids      the kept lines' ids in the input's format: int32_t[cap_lines], or whole u16 / u8 result rows;
 *   out_caps     compact_results 0: their dense capture rows, int32_t[cap_lines * 2 * gx_max_groups(h)].
 * No output may overlap an input.  *n_selected and *bytes_selected (host; bytes, also with utf16) are always set;
 * no output at all (all five NULL) only asks for them.  GX_E_LIMIT when cap_lines
 * or out_bytes_cap is too small: the sizes are set and nothing has been written.  With opts->device_pointers every buffer except
 * want and the two sizes is a device pointer; host buffers are staged to the device and back (there is no CPU path).  Three passes
 * on opts->stream -- flags, scan, copy -- with ONE small synchronisation between scan and copy, where the host reads the two sizes
 * (as gx_pack_results reads its counter; the want mask, 2K + 1 bytes, is copied to the device on every call); opts->no_sync (device pointers) then means: do not wait for the copy pass.  A line of
 * 2^32 code units and more is refused (GX_E_LIMIT).  The device workspace stays on the handle, like gx_results_to_jsonl's. */
int gx_select_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                    const uint8_t* want, uint32_t* out_index, void* out_bytes, void* out_offsets, void* out_ids, int32_t* out_caps,
                    uint64_t cap_lines, uint64_t out_bytes_cap, uint64_t* n_selected, uint64_t* bytes_selected,
                    const gx_batch_opts* opts);

/* The whole-file form, next to gx_text_to_jsonl: raw text -> lines (gx_split_lines semantics) -> the match-and-extract path ->
 * the selected lines' text, concatenated with their terminators.  With want marking outcome K and K+1 .. 2K these are exactly the
 * lines gx_text_to_jsonl writes nothing for: the dead-letter file.  counts (optional, uint64_t[2K + 2], host) receives the
 * histogram of the same pass, *n_lines (optional) the number of lines, *out_size the size of the selected text; out == NULL only
 * asks for the sizes; GX_E_LIMIT when out_cap is too small.  opts: device_pointers (text -- 16-byte aligned -- and out on the
 * device), stream, utf8 (1: the text is UTF-8 and outcomes are those of the decoded Strings; the selected lines are their original bytes).
 * Text of 4 GiB and more must be split by the caller (at a line boundary). */
int gx_text_select(gx_handle* h, const uint8_t* text, uint64_t size, const uint8_t* want, uint8_t* out, uint64_t out_cap,
                   uint64_t* out_size, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* Lines by the VALUES they captured.  The next line of the reference caller's loop is a test on what the extraction found
 * (README.md:26,63-79, on the README definition):
 *     r = gorp.extract(line); if (r != null && Long.parseLong(r.asMap().get("timeTakenInMsec")) >= 500) ...
 * A TERM is one such test on one group of one extraction; its result is test(value) XOR negate, the value being the code units
 * line[begin, end) of the group's capture offsets:
 *   GX_WHERE_SET                     the group took part in the match (Matcher.group(g) != null);
 *   GX_WHERE_EQ / _PREFIX / _SUFFIX / _CONTAINS
 *                                    the value against `text`, code unit by code unit (bytes; 16-bit units with opts->utf16; with
 *                                    utf8 = 1 the literal is UTF-8 bytes).  An empty text is a prefix, a suffix and a part of every
 *                                    value, and equal to the empty value alone;
 *   GX_WHERE_INT_EQ / _LT / _LE / _GT / _GE
 *                                    the value as a number against `number`, parsed as Long.parseLong parses ASCII input: one
 *                                    optional '+' or '-', then one or more digits '0' .. '9', within int64; leading zeros are fine.
 *                                    Anything else fails the test: the empty value, a bare sign, any other unit, overflow -- and a
 *                                    digit that is not ASCII (U+FF11), which Java would accept: the one difference.
 * An unset group fails every test (so with negate it passes). */
enum { GX_WHERE_SET = 0, GX_WHERE_EQ, GX_WHERE_PREFIX, GX_WHERE_SUFFIX, GX_WHERE_CONTAINS,
       GX_WHERE_INT_EQ, GX_WHERE_INT_LT, GX_WHERE_INT_LE, GX_WHERE_INT_GT, GX_WHERE_INT_GE };

typedef struct gx_where_term {
    int32_t  extraction;   /* k in [0, K) */
    int32_t  group;        /* g in [0, gx_num_groups(h, k)) */
    uint32_t op;           /* GX_WHERE_* */
    uint32_t negate;       /* 1: the term holds where the test fails */
    const void* text;      /* HOST pointer (always): the literal in the batch's code units, uint8_t, or uint16_t with opts->utf16 */
    uint32_t text_units;   /* 0 .. 255 */
    int64_t  number;
} gx_where_term;

/* gx_select_lines_where: gx_select_lines with terms.  A line is kept when its outcome index x has want[x] != 0 AND, if x is a matched
 * extraction k that has terms, EVERY term of k holds.  Extractions without terms, unmatched lines and exceptions are decided by want
 * alone: n_terms == 0 is gx_select_lines bit for bit, and the dead-letter mask composes.  Everything else -- inputs, outputs,
 * capacities, the size query, GX_E_LIMIT with nothing written, offsets64, utf16, host staging, stream, no_sync after the one small
 * synchronisation -- is gx_select_lines'; the terms and literals (at most 64 terms of at most 255 units: GX_E_LIMIT beyond) go to the
 * device beside the want mask on every call.  Capture offsets come from caps with int32 ids (caps == NULL with terms: GX_E_ARG), and
 * with compact_results 1 / 2 from the u16 / u8 result rows themselves (0xFFFF / 0xFF: unset).  A SATURATED offset of a compact row
 * (65 534 / 254: gx_batch_opts.compact_results) is taken at face value -- where the batch's *overflow != 0, use dense rows.  The
 * offsets are the caller's input to a kernel: a pair with begin < 0 <= end, end < begin or end beyond the line's
 * offsets[i + 1] - offsets[i] units counts as UNSET and is never dereferenced; no code unit outside [offsets[0], offsets[n]) is
 * read.  utf8 = 1 batches work as they are (byte offsets, UTF-8 literal); utf8 = 2 (offsets in units over a byte buffer) is
 * GX_E_ARG.  A term with extraction, group or op out of range, or text == NULL with text_units > 0, is GX_E_ARG; these refusals need
 * no device (a host-only handle gives them, and GX_E_DEVICE after them: there is no CPU path). */
int gx_select_lines_where(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                          const uint8_t* want, const gx_where_term* terms, uint32_t n_terms, uint32_t* out_index, void* out_bytes,
                          void* out_offsets, void* out_ids, int32_t* out_caps, uint64_t cap_lines, uint64_t out_bytes_cap,
                          uint64_t* n_selected, uint64_t* bytes_selected, const gx_batch_opts* opts);

/* gx_text_select with the same terms: raw text -> lines -> the match-and-extract path (which leaves dense capture rows on the
 * device) -> the text of the lines that want and the terms keep.  counts is the histogram of OUTCOMES, as gx_text_select gives it:
 * the terms do not change it.  With utf8 = 1 a term's text is UTF-8 bytes. */
int gx_text_select_where(gx_handle* h, const uint8_t* text, uint64_t size, const uint8_t* want, const gx_where_term* terms,
                         uint32_t n_terms, uint8_t* out, uint64_t out_cap, uint64_t* out_size, uint64_t* counts, uint64_t* n_lines,
                         const gx_batch_opts* opts);

/* Captured numbers, summarised.  The other thing the reference caller's loop does with a captured number is measure it
 * (README.md:26,63-79, on the README definition):
 *     r = gorp.extract(line); if (r != null) metrics.record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
 * A MEASURE is one group of one extraction, with optional histogram edges.  A line COUNTS for measure m when its outcome is the
 * matched extraction m.extraction and every term of that extraction holds (gx_select_lines_where's rule with every matched extraction
 * wanted; n_terms == 0: every line of the extraction).  Its value -- the code units line[begin, end) of group m.group -- is classed:
 *   unset        the offset pair names no value (the group is unset, or begin < 0 <= end, end < begin, end beyond the line: never
 *                dereferenced);
 *   not_numbers  the value is set and Long.parseLong would throw: the empty value, a bare sign, any other unit, out of int64 -- and
 *                a digit that is not ASCII (U+FF11), which Java would accept: the one difference (GX_WHERE_INT_*'s rule);
 *   numbers      everything else: adds to min, max, the sum and one histogram bucket.
 * lines == numbers + unset + not_numbers.  The sum is EXACT: a 128-bit two's-complement integer (sum_hi : sum_lo) that neither wraps
 * nor saturates, and integer addition makes it the same bits on every run.  An extraction may have several measures (two groups, or
 * one group with different edges). */
typedef struct gx_measure {
    int32_t  extraction;   /* k in [0, K) */
    int32_t  group;        /* g in [0, gx_num_groups(h, k)) */
    const int64_t* edges;  /* HOST pointer (always): histogram edges, strictly ascending; NULL with n_edges == 0 */
    uint32_t n_edges;      /* 0 .. 64 */
} gx_measure;

typedef struct gx_measure_stats {   /* 64 bytes, host */
    uint64_t lines;         /* lines of the extraction that count */
    uint64_t numbers;       /* ... whose value parsed */
    uint64_t unset;         /* ... whose offset pair names no value */
    uint64_t not_numbers;   /* ... whose value is set but is no number */
    int64_t  min, max;      /* over the numbers; numbers == 0: INT64_MAX / INT64_MIN */
    uint64_t sum_lo;        /* the exact sum, bits 0 .. 63 */
    int64_t  sum_hi;        /* ... bits 64 .. 127 */
} gx_measure_stats;

/* gx_capture_stats: stats[n_measures] (host) receives every measure's summary of the batch bytes / offsets / n / ids / caps, which are
 * read exactly as gx_select_lines_where reads them (int32 ids with dense caps, or u16 / u8 result rows with compact_results 1 / 2, a
 * saturated offset taken at face value; offsets64; utf16; utf8 = 1; device_pointers, else the inputs are staged; stream).  hist
 * (host, optional): measure m owns n_edges + 1 consecutive entries, measure after measure in the caller's order; a number v lands in
 * bucket b = the number of edges <= v (bucket 0: v < edges[0]; the last: v >= edges[n_edges - 1]; no edges: one bucket == numbers).
 * One reduction pass and a small second kernel on opts->stream, no atomics in global memory; the call synchronises the stream once,
 * to deliver the results.  GX_E_ARG: measures == NULL or stats == NULL with n_measures > 0, a measure's extraction or group out of
 * range, edges == NULL with n_edges > 0, edges not strictly ascending, every refusal of a term (gx_select_lines_where), terms or
 * measures on dense ids without caps, utf8 = 2, no_sync (the results are host values).  GX_E_LIMIT: more than 64 measures, more
 * than 64 edges in a measure or 1 024 in all, n of 2^32 and more, a line of 2^32 code units and more.  All but the last need no device
 * (a host-only handle gives them, and GX_E_DEVICE after them: there is no CPU path).  n_measures == 0 is legal. */
int gx_capture_stats(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                     const gx_measure* measures, uint32_t n_measures, const gx_where_term* terms, uint32_t n_terms,
                     gx_measure_stats* stats, uint64_t* hist, const gx_batch_opts* opts);

/* The whole-file form, next to gx_text_select_where: raw text -> lines -> the match-and-extract path (which leaves ids and dense
 * capture rows on the device) -> the same summary.  counts (optional, uint64_t[2K + 2], host) is the histogram of outcomes as
 * gx_text_select gives it, *n_lines (optional) the number of lines; both are delivered with n_measures == 0 too.  Limits and options
 * are gx_text_select_where's: text below 4 GiB, device text 16-byte aligned, utf8 0 / 1. */
int gx_text_capture_stats(gx_handle* h, const uint8_t* text, uint64_t size, const gx_measure* measures, uint32_t n_measures,
                          const gx_where_term* terms, uint32_t n_terms, gx_measure_stats* stats, uint64_t* hist, uint64_t* counts,
                          uint64_t* n_lines, const gx_batch_opts* opts);

/* Lines grouped by the text they captured.  The reference caller's remaining everyday move behind the extraction is to key on a
 * captured text (README.md:26,63-79, on the README definition):
 *     r = gorp.extract(line);
 *     if (r != null) { byVerb.merge(r.asMap().get("verb"), 1L, Long::sum);
 *                      latency.computeIfAbsent(r.asMap().get("path"), p -> new Stats()).record(Long.parseLong(r.asMap().get("timeTakenInMsec"))); }
 * A PART names, for the lines of one extraction, the group whose value is the line's KEY and optionally a group that is measured per key
 * as gx_capture_stats measures one.  A line COUNTS when its outcome is a matched extraction that has a part and every term of that
 * extraction holds (gx_capture_stats' rule).  Its key is the code units line[begin, end) of key_group; a pair that names no value (the
 * group is unset, or begin < 0 <= end, end < begin, end beyond the line: never dereferenced) adds to `unset` and gives the line no key.
 * The empty value is a key like any other.  Keys of different parts live in ONE key space: "GET" captured by GetRequest and by
 * OtherRequest is the same key.  Two values are the same key when they have the same number of units and the same units (bytes; 16-bit
 * units with utf16; UTF-8 bytes with utf8 = 1).  Keys leave ORDERED by the first input line that holds them -- the insertion order of a
 * LinkedHashMap filled line by line -- and every result is exact and the same bits on every run.  This is also the dictionary encoding
 * of the column: the distinct values plus a key number per line. */
#define GX_GROUP_WEAK_HASH 1u   /* test hook (as GX_CREATE_PROGRAMS is): the hash is cut to its low 3 bits, so distinct values share tag
                                   AND first slot; results are identical, only slower */

typedef struct gx_group_part {  /* the lines of ONE extraction: which group is the key, which (if any) the number */
    int32_t extraction;         /* k in [0, K); at most one part per extraction */
    int32_t key_group;          /* g in [0, gx_num_groups(h, k)) */
    int32_t value_group;        /* -1: count only; else a group parsed as gx_capture_stats parses one */
    uint32_t reserved;          /* 0 */
} gx_group_part;

typedef struct gx_group_out {   /* every pointer optional; device memory with opts->device_pointers, else host */
    void*     key_units;        /* the distinct values, one behind the other, in the batch's code units (u8; u16 with utf16) */
    uint64_t  key_units_cap;
    void*     key_offsets;      /* n_keys + 1, uint32 or uint64 as opts->offsets64: key j is key_units[key_offsets[j], key_offsets[j+1]) */
    uint32_t* key_first_line;   /* the first input line that holds key j: keys are ORDERED by it */
    uint64_t* key_lines;        /* lines that hold key j */
    gx_measure_stats* key_stats;/* per key, over its lines whose part has a value_group (exact 128-bit sum; no histogram) */
    uint32_t* line_key;         /* n entries: the key number of every input line, 0xFFFFFFFF for a line that has none */
    uint64_t  max_keys;         /* capacity of the four per-key arrays (key_offsets: max_keys + 1) */
} gx_group_out;

typedef struct gx_group_totals {/* host, always */
    uint64_t n_keys, key_units; /* what the outputs need */
    uint64_t lines;             /* lines that count (their extraction has a part and every term of it holds) */
    uint64_t keyed, unset;      /* ... whose key pair names a value / names none: lines == keyed + unset */
    uint64_t exact;             /* 1: n_keys and key_units are exact; 0: the table overflowed, n_keys is only a lower bound */
} gx_group_totals;

/* gx_group_lines: the batch bytes / offsets / n / ids / caps is read exactly as gx_capture_stats reads it (row formats, offsets64,
 * utf16, utf8 = 1, device_pointers or staging, stream).  key_stats[j] summarises key j's lines whose part has a value_group: lines ==
 * numbers + unset + not_numbers, min / max INT64_MAX / INT64_MIN without a number, the sum exact; where no part has a value group
 * key_stats must be NULL.  The keys are found in a hash table on the device of the smallest power of two >= max(64, 2 * max_keys) slots.
 * With every output pointer NULL (or out == NULL) the call is the size query: only *totals is delivered, and max_keys is still read, as
 * the table's size.  If a per-key array is given and n_keys > max_keys, or key_units is given and totals->key_units > key_units_cap, the
 * call returns GX_E_LIMIT, writes nothing to any output and fills *totals.  If a line finds no free slot the call returns GX_E_LIMIT
 * with exact = 0 and n_keys = slots + 1; the number of lines is always a sufficient max_keys.  The call synchronises the stream once,
 * where the host reads the totals; with host outputs a second wait delivers them.
 * GX_E_ARG: parts == NULL with n_parts > 0, totals == NULL, a part's extraction or group out of range, two parts for one extraction,
 * reserved != 0, unknown flag bits, key_stats without a value_group, every refusal of a term (gx_select_lines_where), parts or terms on
 * dense ids without caps, utf8 = 2, no_sync.  GX_E_LIMIT: more than 64 parts, n of 2^32 - 1 and more, max_keys above 2^30, a line of
 * 2^32 code units and more (or offsets that go backwards).  All need no device (a host-only handle gives them, and GX_E_DEVICE after
 * them: there is no CPU path) but the last with device_pointers, where the offsets lie on the device and the build pass finds it.
 * n_parts == 0 is legal: no keys, all zeros.
 * With device_pointers the emit pass is left running on opts->stream when the call returns (stream order delivers the outputs); the
 * handle's next gx_group_lines on another stream waits for it, and the batch must stay unchanged until it has run. */
int gx_group_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                   const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                   const gx_group_out* out, gx_group_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_capture_stats' chain with the grouping at its end: raw text -> lines -> the match-and-extract path ->
 * the same result.  counts (optional, uint64_t[2K + 2], host) and *n_lines (optional) as gx_text_capture_stats delivers them, with
 * n_parts == 0 too.  out->line_key, if given, has one entry per line of the text (the size query delivers *n_lines).  Limits and options
 * are gx_text_capture_stats': text below 4 GiB, device text 16-byte aligned, utf8 0 / 1.  Like every gx_text_* call it returns with
 * all its work on opts->stream done, with device_pointers too: its passes read the lines' offsets, ids and capture rows from the handle's
 * buffers, which the next whole-file call reuses. */
int gx_text_group_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                        const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* out,
                        gx_group_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* Lines ranked by a number they captured.  The reference caller's question "which requests were the slowest?" (README.md:26,63-79, on
 * the README definition) is
 *     r = gorp.extract(line); if (r != null) results.add(r); ... sorted(results, by Long.parseLong(timeTakenInMsec)).take(N)
 * A PART names, for the lines of one extraction, the group whose value is the line's number; all parts share ONE number space ("the
 * slowest requests, GetRequest or OtherRequest").  A line COUNTS when its outcome is a matched extraction that has a part and every
 * term of that extraction holds (gx_capture_stats' rule), and its value is classed exactly as gx_capture_stats classes one: unset, not a
 * number, or a number.  Only numbers are candidates.  The result is the n_top = min(n_wanted, numbers) candidates ordered by (value
 * descending, input line ascending) -- with GX_TOP_SMALLEST by (value ascending, input line ascending) -- so ties at the cut go to the
 * earliest lines.  Every output is exact and the same bits on every run. */
#define GX_TOP_SMALLEST 1u
#define GX_TOP_MAX_LINES 4096u  /* the cap on n_wanted */

typedef struct gx_top_part {    /* the lines of ONE extraction: which group is the number */
    int32_t extraction;         /* k in [0, K); at most one part per extraction */
    int32_t value_group;        /* g in [0, gx_num_groups(h, k)), parsed as gx_capture_stats parses one */
} gx_top_part;

typedef struct gx_top_totals {  /* host, always */
    uint64_t lines, numbers, unset, not_numbers;   /* as gx_measure_stats, over all parts: lines == numbers + unset + not_numbers */
    uint64_t n_top, units_top;  /* what the outputs need: delivered lines, and their code units */
    int64_t  last_value;        /* value of the last delivered line; 0 when n_top == 0 */
    uint64_t ties_left;         /* numbers equal to last_value that were NOT delivered */
} gx_top_totals;

/* gx_top_lines: the batch bytes / offsets / n / ids / caps is read exactly as gx_capture_stats reads it (row formats, where a saturated
 * compact offset is taken at face value; offsets64, utf16, utf8 = 1, device_pointers or staging, stream).  The outputs, their capacities
 * and the size query behave as gx_select_lines' do: every output pointer is optional -- out_index (the delivered lines' input line
 * numbers), out_values (their numbers), out_bytes / out_offsets (their code units and n_top + 1 offsets of the input's width), out_ids
 * and out_caps (their result rows), all in rank order; with all of them NULL only *totals is delivered.  If a per-line output is given
 * and n_top > cap_lines, or out_bytes is given and the delivered text is larger than out_bytes_cap bytes, the call returns GX_E_LIMIT,
 * writes nothing to any output and fills *totals; cap_lines >= n_wanted always suffices.  The call synchronises the stream once, where
 * the host reads the totals and checks the capacities; with host outputs a second wait delivers them.  With device_pointers the emit
 * pass is left running on opts->stream when the call returns (stream order delivers the outputs); the handle's next gx_top_lines on
 * another stream waits for it, and the batch must stay unchanged until it has run.
 * GX_E_ARG: totals == NULL, parts == NULL with n_parts > 0, a part's extraction or group out of range, two parts for one extraction,
 * unknown flag bits, every refusal of a term (gx_select_lines_where), parts or terms on dense ids without caps, utf8 = 2, no_sync.
 * GX_E_LIMIT: more than 64 parts, n_wanted > GX_TOP_MAX_LINES, n of 2^32 - 1 and more, a line of 2^32 code units and more (or offsets
 * that go backwards).  All need no device (a host-only handle gives them, and GX_E_DEVICE after them: there is no CPU path) but the
 * last with device_pointers, where the offsets lie on the device and the keys pass finds it.  n_parts == 0 and n_wanted == 0 are legal
 * and give no lines (n_wanted == 0 still fills the four counts). */
int gx_top_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                 const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t n_wanted,
                 uint32_t flags, uint32_t* out_index, int64_t* out_values, void* out_bytes, void* out_offsets, void* out_ids,
                 int32_t* out_caps, uint64_t cap_lines, uint64_t out_bytes_cap, gx_top_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_capture_stats' chain with the ranking at its end: raw text -> lines -> the match-and-extract path -> the
 * same result.  The chosen lines' text leaves in `out` as gx_text_select_where delivers kept lines (each with its terminator as the
 * text has it), in rank order; out_index / out_values (optional, room for n_wanted entries) are the lines' numbers in the text and their
 * values.  *out_size: the bytes the text needs (out == NULL: the size query).  counts (optional, uint64_t[2K + 2], host) and *n_lines
 * (optional) as gx_text_capture_stats delivers them.  Limits and options are gx_text_capture_stats': text below 4 GiB, device text
 * 16-byte aligned, utf8 0 / 1.  Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_top_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts,
                      const gx_where_term* terms, uint32_t n_terms, uint32_t n_wanted, uint32_t flags, uint32_t* out_index,
                      int64_t* out_values, uint8_t* out, uint64_t out_cap, uint64_t* out_size, gx_top_totals* totals, uint64_t* counts,
                      uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- percentiles of a number the lines captured --------------------------------------------------------------------------------
 * The reference's caller asks for the median and the p95 / p99 of a captured number right behind the extraction (README.md:26,63-79:
 * the results' timeTakenInMsec).  Parts are gx_top_part records with gx_top_lines' meaning -- at most one per extraction, one number
 * space -- and a line COUNTS, and its value is classed unset / not a number / number, exactly as there.  The numbers are the
 * population.  A quantile is num / den, and its rank is nearest-rank in integers alone, with p = (uint64_t)num * numbers:
 *     rank = p / den + (p % den != 0), a rank of 0 raised to 1
 * so 1 <= rank <= numbers, num == 0 is the minimum and num == den the maximum: sorted(values)[ceil(q * numbers) - 1].  No floating
 * point appears anywhere.  Per quantile: value, the rank-th smallest number; rank; below, the numbers strictly below value; equal,
 * the numbers equal to it (below < rank <= below + equal).  With numbers == 0 every entry is all zeros.  Quantiles may come in any
 * order and may repeat; each gets its own entry, in input order.  Every output is exact and the same bits on every run. */
#define GX_QUANTILE_MAX 16u
typedef struct gx_quantile     { uint32_t num, den; } gx_quantile;          /* q = num / den; den >= 1, num <= den */
typedef struct gx_quantile_out { int64_t value; uint64_t rank, below, equal; } gx_quantile_out;   /* 32 bytes, host */
typedef struct gx_quantile_totals { uint64_t lines, numbers, unset, not_numbers; } gx_quantile_totals;   /* 32 bytes, host */

/* gx_capture_quantiles: the batch bytes / offsets / n / ids / caps is read exactly as gx_top_lines reads it (row formats, offsets64,
 * utf16, utf8 = 1, device_pointers or staging, stream).  out[n_quantiles] and *totals are host values.  The call synchronises the
 * stream once; the host reads nothing between the passes, and nothing of the call is left running when it returns.
 * GX_E_ARG: totals == NULL, quantiles == NULL or out == NULL with n_quantiles > 0, den == 0, num > den, every refusal of parts and terms
 * that gx_top_lines makes, parts or terms on dense ids without caps, utf8 = 2, no_sync.  GX_E_LIMIT: n_quantiles > GX_QUANTILE_MAX, more
 * than 64 parts, n of 2^32 - 1 and more, a line of 2^32 code units and more (or offsets that go backwards).  All need no device (a
 * host-only handle gives them, and GX_E_DEVICE after them: there is no CPU path) but the last with device_pointers, where the keys
 * pass finds it.  n == 0 and n_parts == 0 are legal and give zeros; n_quantiles == 0 fills the totals alone. */
int gx_capture_quantiles(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                         const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                         const gx_quantile* quantiles, uint32_t n_quantiles, gx_quantile_out* out, gx_quantile_totals* totals,
                         const gx_batch_opts* opts);

/* The whole-file form, gx_text_capture_stats' chain with the quantiles at its end: raw text -> lines -> the match-and-extract path ->
 * the same result.  counts (optional, uint64_t[2K + 2], host), *n_lines (optional), limits and options are gx_text_capture_stats'. */
int gx_text_capture_quantiles(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts,
                              const gx_where_term* terms, uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles,
                              gx_quantile_out* out, gx_quantile_totals* totals, uint64_t* counts, uint64_t* n_lines,
                              const gx_batch_opts* opts);

/* ---- percentiles of a captured number per captured text -------------------------------------------------------------------------
 * The question an operator asks of a request log: p50 / p95 / p99 of timeTakenInMsec per path.  The reference's caller answers it
 * right behind the extraction with a map of lists (README.md:26,63-79):
 *     byPath.computeIfAbsent(r.asMap().get("path"), p -> new ArrayList<>()).add(Long.parseLong(r.asMap().get("timeTakenInMsec")));
 *     ... sorted(list)[ceil(q * list.size()) - 1] per key
 * gx_group_quantiles is gx_group_lines plus ONE output; nothing of gx_group_lines is reinterpreted.  Parts, terms, flags, out, totals,
 * row formats, offsets64, utf16, utf8 = 1, staging or device_pointers, the stream, the size query, GX_E_LIMIT with nothing written and
 * the overflowed table (exact = 0) are gx_group_lines'.  With n_quantiles == 0 the call delivers what gx_group_lines delivers, bit for
 * bit, and key_quantiles is not touched.
 * The quantiles are gx_quantile records with gx_capture_quantiles' rule (nearest rank in integers alone), at most GX_QUANTILE_MAX, in
 * any order, repeats allowed.  Key j's POPULATION is the numbers among key j's lines whose part has a value_group: exactly the lines
 * counted in key_stats[j].numbers.  A line whose key pair names no value belongs to no key; a part with value_group = -1 adds lines to
 * its keys and nothing to their populations.
 * key_quantiles (optional) holds n_keys x n_quantiles rows, key-major, the keys in gx_group_lines' order; its capacity is
 * out->max_keys x n_quantiles rows (out == NULL: 0); device memory with device_pointers, else host, like the other per-key arrays.
 * Row (j, q): value, the rank-th smallest number of key j; rank; below, the numbers of key j strictly below value; equal, those equal
 * to it (below < rank <= below + equal <= key_stats[j].numbers).  A key without numbers gets all-zero rows.  Every result is exact
 * and the same bits on every run.  key_quantiles == NULL with n_quantiles > 0 is legal: the size query, or the keys alone.
 * GX_E_ARG, besides gx_group_lines': quantiles == NULL with n_quantiles > 0, den == 0, num > den.  GX_E_LIMIT, besides gx_group_lines':
 * n_quantiles > GX_QUANTILE_MAX; key_quantiles given with n_keys > max_keys (nothing is written to any output, *totals is filled).
 * All before the device is looked at: a host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).
 * The call synchronises the stream once, where the host reads the totals and, in the same wait, what the sort's digit plan needs; with
 * host outputs a second wait delivers them.  With device_pointers the remaining passes are left running on opts->stream; the handle's
 * next gx_group_lines / gx_group_quantiles on another stream waits for them. */
int gx_group_quantiles(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                       const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                       const gx_quantile* quantiles, uint32_t n_quantiles, uint32_t flags, const gx_group_out* out,
                       gx_quantile_out* key_quantiles, gx_group_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the per-key quantiles at its end; counts, *n_lines, limits and options are
 * gx_text_group_lines'.  Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_quantiles(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                            const gx_where_term* terms, uint32_t n_terms, const gx_quantile* quantiles, uint32_t n_quantiles,
                            uint32_t flags, const gx_group_out* out, gx_quantile_out* key_quantiles, gx_group_totals* totals,
                            uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* Keys ranked by their lines or by the numbers their lines captured.  The reference caller's question "which keys are the biggest?"
 * (README.md:26,63-79), on the map gx_group_lines builds:
 *     byPath.merge(r.asMap().get("path"), 1L, Long::sum);          // or .record(Long.parseLong(timeTakenInMsec))
 *     ... byPath.entrySet().stream().sorted(comparingByValue().reversed()).limit(10)
 * Keys, parts, terms, which lines count, key equality, the one key space and the key numbers (order of first line) are gx_group_lines';
 * nothing of that is reinterpreted.  Every key has a RANK VALUE, a signed 128-bit integer chosen by rank_by:
 *     GX_RANK_LINES    key_lines[j]                        every key is a candidate
 *     GX_RANK_NUMBERS  key_stats[j].numbers                every key
 *     GX_RANK_SUM      the exact sum sum_hi : sum_lo       keys with numbers >= 1
 *     GX_RANK_MAX      key_stats[j].max, sign-extended     keys with numbers >= 1
 *     GX_RANK_MIN      key_stats[j].min, sign-extended     keys with numbers >= 1
 * The result is the n_top = min(n_wanted, candidates) candidates ordered by (rank value descending, key number ascending) -- with
 * GX_TOP_GROUPS_SMALLEST by (rank value ascending, key number ascending) -- so ties at the cut go to the keys that appeared first:
 * gx_top_lines' tie rule, one level up.  Every output is exact and the same bits on every run; there is no floating point anywhere.
 * Ranking by the mean or by a per-key quantile is not offered. */
enum { GX_RANK_LINES = 0, GX_RANK_NUMBERS, GX_RANK_SUM, GX_RANK_MAX, GX_RANK_MIN };
#define GX_TOP_GROUPS_SMALLEST 2u      /* GX_GROUP_WEAK_HASH (1u) is accepted in the same flags word; GX_TOP_SMALLEST is also 1u and is NOT used here */
#define GX_TOP_GROUPS_MAX 4096u        /* the cap on n_wanted */

typedef struct gx_top_groups_out {     /* every pointer optional; device memory with opts->device_pointers, else host; all in RANK order */
    void*     key_units;  uint64_t key_units_cap;
    void*     key_offsets;             /* n_top + 1, uint32 / uint64 as opts->offsets64 */
    uint32_t* key_number;              /* the key's number in gx_group_lines' order (what gx_group_lines' line_key holds) */
    uint32_t* key_first_line;
    uint64_t* key_lines;
    gx_measure_stats* key_stats;       /* NULL unless a part has a value_group */
    uint32_t* line_rank;               /* n entries: the rank 0 .. n_top-1 of the line's key, 0xFFFFFFFF: no key, or key not delivered */
    uint64_t  cap_keys;                /* capacity of the per-key arrays (key_offsets: cap_keys + 1); n_wanted always suffices */
} gx_top_groups_out;

typedef struct gx_top_groups_totals {  /* host, always */
    gx_group_totals group;             /* exactly what gx_group_lines reports for the same call */
    uint64_t candidates, n_top, units_top;
    uint64_t last_lo; int64_t last_hi; /* rank value of the last delivered key, two's complement as sum_lo / sum_hi; 0 when n_top == 0 */
    uint64_t ties_left;                /* candidates with that rank value that were not delivered */
} gx_top_groups_totals;

/* gx_top_groups: the batch is read exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16;
 * utf8 = 1; staging or device_pointers; the stream).  max_keys sizes the hash table exactly as gx_group_out.max_keys does: the smallest
 * power of two >= max(64, 2 * max_keys) slots, and n always suffices; an overflowed table is GX_E_LIMIT with group.exact = 0, and nothing
 * is written.  With every output NULL, or out == NULL, the call is the size query: only *totals is delivered.  A per-key array with
 * n_top > cap_keys, or key_units with units_top > key_units_cap, returns GX_E_LIMIT: every output stays untouched and *totals is filled.
 * The host waits on the stream twice before any output is written -- for gx_group_lines' totals, then for what the select found -- and
 * with host outputs a third wait delivers them; with device_pointers the emit over the chosen keys is left running on opts->stream
 * when the call returns, and the handle's next group call on another stream waits for it.
 * GX_E_ARG, besides every refusal gx_group_lines makes: rank_by out of range, rank_by != GX_RANK_LINES when no part has a value group,
 * key_stats without a value group, unknown flag bits, totals == NULL, no_sync, utf8 = 2.  GX_E_LIMIT: n_wanted > GX_TOP_GROUPS_MAX, plus
 * gx_group_lines' limits.  All of these come before the device is looked at (a host-only handle gives them, and GX_E_DEVICE after them:
 * there is no CPU path), except what gx_group_lines itself can only see on the device.  n_parts == 0, n_wanted == 0 and n == 0 are
 * legal; with n_wanted == 0 the totals are still filled. */
int gx_top_groups(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                  const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t rank_by,
                  uint32_t n_wanted, uint64_t max_keys, uint32_t flags, const gx_top_groups_out* out, gx_top_groups_totals* totals,
                  const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the ranking at its end; counts and *n_lines are delivered as there, and
 * out->line_rank has one entry per line of the text.  Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_top_groups(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                       const gx_where_term* terms, uint32_t n_terms, uint32_t rank_by, uint32_t n_wanted, uint64_t max_keys,
                       uint32_t flags, const gx_top_groups_out* out, gx_top_groups_totals* totals, uint64_t* counts, uint64_t* n_lines,
                       const gx_batch_opts* opts);

/* gx_partition_lines: every sink's lines at once.  Inputs, outputs, formats and options are exactly gx_select_lines'; the kept lines
 * -- those whose outcome index x <= 2K has want[x] != 0; want == NULL keeps every outcome 0 .. 2K -- leave ordered by (outcome index,
 * input line number): a stable partition.  The outcome-0 lines come first, then outcome 1's, and so on, in input order inside each
 * group; bin 2K + 1 is counted out and never written.  The result is an ordinary CSR batch (out_bytes / out_offsets, out_ids and
 * out_caps or whole result rows, out_index = the lines' numbers in the input) and composes with gx_extract_batch,
 * gx_results_to_jsonl and gx_select_lines as any other.
 *   group_lines  (host, optional, uint64_t[2K + 3]) an exclusive prefix: outcome x's lines are the output lines
 *                group_lines[x] .. group_lines[x + 1]; an outcome that is not wanted and bin 2K + 1 are empty groups, and
 *                group_lines[2K + 2] == *n_out;
 *   group_units  (host, optional, uint64_t[2K + 3]) the same in code units of out_bytes: out_offsets read at those lines, so that a
 *                caller slices out_bytes per sink without touching device memory.
 * *n_out and *bytes_out (host; bytes, also with utf16) and the two group arrays are always set; no output at all (all five NULL) only
 * asks for them.  GX_E_LIMIT when cap_lines or out_bytes_cap is too small: the sizes are set and nothing has been written.  The passes
 * on opts->stream -- keys, a stable radix sort of the line numbers (one six-bit digit for K <= 31, two up to K = 2047, three beyond),
 * scan, copy -- read the id column once, whatever K is, and there is ONE small synchronisation, between scan and copy, where the host
 * reads the sizes and the groups; opts->no_sync (device pointers) then means: do not wait for the copy pass.  n of 2^32 and more and a
 * line of 2^32 code units and more are refused (GX_E_LIMIT).  The device workspace stays on the handle, shared with gx_select_lines:
 * 32 bytes per INPUT line (destination offsets 8, two key and two line-number arrays of the sort 16, lengths before and behind the
 * sort 8; gx_select_lines needs 21) plus 768 bytes of counts per 2 048 lines -- 320 MB after a batch of 10 M lines, until gx_destroy.
 * Host buffers (device_pointers = 0) are staged; the text only when out_bytes is given: a size query sends the ids and offsets alone. */
int gx_partition_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                       const uint8_t* want, uint32_t* out_index, void* out_bytes, void* out_offsets, void* out_ids, int32_t* out_caps,
                       uint64_t cap_lines, uint64_t out_bytes_cap, uint64_t* group_lines, uint64_t* group_units, uint64_t* n_out,
                       uint64_t* bytes_out, const gx_batch_opts* opts);

/* Every key's lines together.  The reference caller's remaining everyday move on a captured text (README.md:26,63-79) is
 *     r = gorp.extract(line);
 *     if (r != null) byRequest.computeIfAbsent(r.asMap().get("requestId"), k -> new ArrayList<>()).add(line);
 * -- Collectors.groupingBy on a captured text: every request's, session's or trace's lines together, in the order they were logged; the
 * keys with exactly one line are the requests that have a start line and no end line.  gx_group_lines gets as far as line_key; this call
 * does the regrouping on the device, as gx_partition_lines does it by outcome.
 * INHERITED from gx_group_lines, and nothing of it is reinterpreted: keys, parts and terms, which lines count, key equality and the one
 * key space, the key numbers (order of first line), max_keys sizing the table.  `keys` is gx_group_lines' own output struct and delivers
 * exactly what that call would, for every key, kept or not.
 * KEPT: key j is kept when max(min_lines, 1) <= key_lines[j], and either max_lines == 0 or key_lines[j] <= max_lines.  A line is kept when
 * it has a key and that key is kept.
 * ORDER: the kept lines leave ordered by (key number, input line number) -- sessions in order of their first line, lines in input order
 * inside each: what a LinkedHashMap<String, List<String>> filled line by line holds.  A key that is not kept is an empty range in the two
 * prefix arrays; key_out_lines[n_keys] == lines_out.
 * COPIES: each line is copied as gx_select_lines copies one: units exactly, terminator included.  out_ids and out_caps hold the lines'
 * ids or whole result rows in the input's format, so the result is an ordinary batch for every other call.
 * EXACT: every output is exact and the same bits on every run: ranks come from ballots and scans, and no output depends on wave timing. */
#define GX_BY_KEY_ALL_DIGITS 2u   /* test hook, accepted beside GX_GROUP_WEAK_HASH (1u): sort all five key-number digits whatever n_keys is;
                                     results identical, only slower */

typedef struct gx_by_key_out {    /* every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* out_index;          /* gx_partition_lines' five outputs, same meaning, same formats: the kept lines as a new CSR batch */
    void*     out_bytes;
    void*     out_offsets;
    void*     out_ids;
    int32_t*  out_caps;
    uint64_t  cap_lines, out_bytes_cap;
    uint64_t* key_out_lines;      /* keys->max_keys + 1: exclusive prefix; key j's lines are output lines [key_out_lines[j], key_out_lines[j+1]) */
    uint64_t* key_out_units;      /* the same in code units of out_bytes (out_offsets read at those lines) */
} gx_by_key_out;

typedef struct gx_by_key_totals { /* host, always */
    gx_group_totals group;        /* exactly what gx_group_lines reports for the same call */
    uint64_t keys_kept, lines_out, units_out;
} gx_by_key_totals;

/* gx_lines_by_key: the batch is read exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16;
 * utf8 = 1; staging or device_pointers; the stream).  cap_lines is the capacity of out_index, out_ids, out_caps (lines) and out_offsets
 * (cap_lines + 1, the width of the input's offsets); out_bytes_cap is in BYTES, with utf16 too.  key_out_lines and key_out_units hold
 * n_keys + 1 entries each and are sized by keys->max_keys + 1 (keys == NULL: max_keys 0).
 * HOST WAITS: ONE host wait before any output -- the wait in which gx_group_lines reads its totals also reads keys_kept, lines_out and
 * units_out, computed by a pass behind the build on the same stream from the per-slot line counts of the table and the lengths in the
 * offsets.  With host outputs a second wait delivers them.  With device_pointers the passes (compaction, a stable radix sort of the kept
 * lines by key number with ceil(bits(n_keys - 1) / 6) six-bit digits -- none for one key, five for 2^30 keys --, scan, copy) are left
 * running on opts->stream when the call returns, as gx_group_lines leaves its emit; the handle's next group call on another stream
 * waits for them, and the batch must stay unchanged until they have run.
 * SIZE QUERY: all of out's pointers NULL, or out == NULL: only *totals is delivered, and with `keys` whatever gx_group_lines would
 * deliver.
 * GX_E_LIMIT: cap_lines < lines_out (with any per-line output), out_bytes_cap too small, key_out_lines / key_out_units with n_keys >
 * keys->max_keys, 32-bit out_offsets with 2^32 units and more: no output of out and none of keys is written, and *totals is filled;
 * and gx_group_lines' own limits, including the overflowed table with group.exact = 0.
 * GX_E_ARG: every refusal gx_group_lines makes; max_lines != 0 && min_lines > max_lines; unknown flag bits; totals == NULL; no_sync;
 * utf8 = 2; out_caps on compact rows; an output overlapping an input (an output's capacity in bytes -- of at most n lines, whatever cap_lines says -- against bytes, offsets, ids and
 * caps; of device bytes only the first unit is known before the device is looked at).  All of these come before the device is looked
 * at: a host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).  n == 0 and n_parts == 0 are legal and give all
 * zeros (out_offsets and the two prefix arrays: their one entry).  With lines_out == 0 out_offsets[0] = 0, the two prefix arrays are all
 * zeros and nothing else is written.
 * The device workspace stays on the handle, a buffer of its own beside gx_group_lines': 33 bytes per INPUT line (the scan of the kept
 * flags, later the destination offsets 8; two key-number and two line-number arrays of the sort 16; the lengths by line and in output
 * order 8; the flags 1) plus 768 bytes of counts per 2 048 lines, until gx_destroy. */
int gx_lines_by_key(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                    const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint64_t min_lines,
                    uint64_t max_lines, uint32_t flags, const gx_group_out* keys, const gx_by_key_out* out, gx_by_key_totals* totals,
                    const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the regrouping at its end: raw text -> lines -> the match-and-extract path ->
 * the regrouping.  out (out_cap bytes) receives the kept lines' original bytes one behind the other, as gx_text_select writes them;
 * out_offsets (optional, lines_out + 1 entries, uint32 whatever opts->offsets64 says: the text is below 4 GiB) delimits them -- a last line of the text without a
 * terminator is copied as it is and may now lie in the middle, so the output is cut at out_offsets, not at line ends; out_index
 * (optional, lines_out entries) holds line numbers of the text.  out_offsets and out_index are sized by the size query (out, out_offsets,
 * out_index, key_out_lines and key_out_units all NULL); *n_lines entries (+ 1) always suffice.  counts and *n_lines as
 * gx_text_group_lines delivers them.  Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_lines_by_key(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                         const gx_where_term* terms, uint32_t n_terms, uint64_t min_lines, uint64_t max_lines, uint32_t flags,
                         const gx_group_out* keys, uint8_t* out, uint64_t out_cap, void* out_offsets, uint32_t* out_index,
                         uint64_t* key_out_lines, uint64_t* key_out_units, gx_by_key_totals* totals, uint64_t* counts, uint64_t* n_lines,
                         const gx_batch_opts* opts);

/* ---- A whole batch ordered by a number its lines captured, on the device (gx_sort_lines) ----
 * The reference's caller who reads two hosts' logs, or a log written by several threads, sorts first (README.md:26,63-79):
 *     results.sort(Comparator.comparingLong(r -> Instant.parse(r.asMap().get("ts")).toEpochMilli()));
 * gx_top_lines ranks by a captured number but delivers GX_TOP_MAX_LINES lines at most; this call orders the whole batch.  Parts are
 * gx_top_part records with gx_top_lines' meaning -- at most one per extraction, one number space -- and values are read under their
 * gx_number_format (ISO-8601, CLF, decimals: gx_set_number_format).  Terms are gx_where_terms.
 * CLASSES.  A line is STAMPED (class 0) when it counts by gx_top_lines' rule and its value is a number.  With GX_SORT_CARRY a line that
 * is not stamped -- unmatched, an exception, an extraction without a part, a failed term, an unset group, a value that is no number, all
 * alike -- and that has a stamped line somewhere before it in the batch is CARRIED (class 1): it takes the number of the nearest earlier
 * stamped line, as a stack trace belongs to the line above it.  Every other line is REST (class 2): without GX_SORT_CARRY every line that
 * is not stamped, with it only the lines before the first stamped line.
 * ORDER.  The stamped and carried lines (the ENTRIES) leave first, ordered by (value ascending, input line ascending), with
 * GX_SORT_DESCENDING by (value descending, input line ascending): ties go by input line in both directions, so a header and the lines it
 * carries leave together and in order, and two records with equal stamps leave in input order.  With GX_SORT_REST_LAST the rest lines
 * follow in input order; without it they are dropped.
 * COPIES: each line is copied as gx_select_lines copies one: units exactly, terminator included.  out_ids and out_caps hold the lines'
 * ids or whole result rows in the input's format, so the result is an ordinary batch for every other call.
 * EXACT: every output is exact and the same bits on every run: places come from scans, ranks from ballots, and there is no atomic
 * operation on global memory in any pass. */
#define GX_SORT_DESCENDING 1u
#define GX_SORT_CARRY      2u
#define GX_SORT_REST_LAST  4u
#define GX_SORT_ALL_DIGITS 8u   /* test hook: sort all eleven six-bit digits of the key whatever the keys are; results identical, only slower */

typedef struct gx_sort_out {    /* every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* out_index;        /* the delivered lines' input line numbers */
    int64_t*  out_values;       /* their numbers (a carried line: its header's); 0 for a rest line */
    uint8_t*  out_class;        /* 0 own number, 1 carried, 2 rest */
    void*     out_bytes;        /* gx_partition_lines' outputs, same meaning, same formats: the delivered lines as a new CSR batch */
    void*     out_offsets;
    void*     out_ids;
    int32_t*  out_caps;
    uint64_t  cap_lines, out_bytes_cap;
} gx_sort_out;

typedef struct gx_sort_totals { /* host, always */
    uint64_t lines, numbers, unset, not_numbers;   /* gx_top_totals' four, same meaning: lines == numbers + unset + not_numbers */
    uint64_t carried, rest;                        /* the carried lines; the rest lines, delivered or dropped */
    uint64_t lines_out, units_out;                 /* what the outputs need: numbers + carried (+ rest with GX_SORT_REST_LAST), and their code units */
    int64_t  first_value, last_value;              /* of the entries in output order; 0 without one */
    uint32_t n_passes;                             /* the digits the sort takes: those in which two entries' keys differ (eleven with GX_SORT_ALL_DIGITS) */
    uint32_t already_ordered;                      /* 1: no entry's key is below the key of the entry before it in line order (also without entries) */
} gx_sort_totals;

/* gx_sort_lines: the batch is read exactly as gx_top_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1;
 * staging or device_pointers; the stream).  cap_lines is the capacity of out_index, out_values, out_class, out_ids, out_caps (lines) and
 * out_offsets (cap_lines + 1, the width of the input's offsets); out_bytes_cap is in BYTES, with utf16 too.
 * HOST WAITS: ONE host wait before any output.  Before it run gx_top_lines' keys pass, a scan of its candidate flags, the compaction of
 * the stamped keys, the entries pass (one lane per line: class, place, the (key, line) pair, the length) and a one-workgroup totals pass;
 * in the wait the host reads the totals and checks the capacities.  Behind it, when outputs are wanted: a stable radix sort of the
 * entries over the six-bit digits in which their keys' OR and AND differ (none for fewer than two distinct keys, eleven at most), the
 * values, classes and lengths in output order, a scan, the copy.  With host outputs a second wait delivers them.  With device_pointers
 * those passes are left running on opts->stream behind an event of this call's own; the handle's next gx_sort_lines on another stream
 * waits for them, and the batch must stay unchanged until they have run.
 * SIZE QUERY: out == NULL, or all of out's pointers NULL: only *totals is delivered.
 * GX_E_LIMIT with *totals filled and no output written: cap_lines < lines_out (with any per-line output), out_bytes_cap too small, 32-bit
 * out_offsets with 2^32 units and more.
 * GX_E_ARG, before the device is looked at: every refusal gx_top_lines makes of parts and terms; unknown flag bits; totals == NULL;
 * no_sync; utf8 = 2; parts or terms on dense ids without caps; out_caps on compact rows or without caps; an output overlapping an input
 * (an output's capacity in bytes -- of at most n lines, whatever cap_lines says -- against bytes, offsets, ids and caps; of device bytes
 * only the first unit is known before the device is looked at).  GX_E_LIMIT, likewise before the device is looked at: more than 64
 * parts or terms; n above 2^30 (what the pair sort's kernels state); with host offsets a line of 2^32 code units and more, or offsets
 * that go backwards (with device_pointers the entries pass finds it).  A host-only handle gives all of these, and GX_E_DEVICE after them
 * (there is no CPU path).
 * n == 0 and n_parts == 0 are legal; with n_parts == 0 every line is a rest line, and GX_SORT_REST_LAST then copies the batch through
 * unchanged.  With lines_out == 0 out_offsets[0] = 0 and nothing else is written.
 * The device workspace stays on the handle, a buffer of its own: 50 bytes per INPUT line (the keys, later the sort's second key array 8;
 * the stamped keys in line order 8; the sort's first key array 8; its two line-number arrays 8; the scan of the candidate flags, later
 * the destination offsets 8; the lengths by line and in output order 8; the flags 1; the classes 1) plus 768 bytes of counts per 2 048
 * lines, until gx_destroy. */
int gx_sort_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                  const gx_top_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                  const gx_sort_out* out, gx_sort_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_top_lines' chain with the ordering at its end: raw text -> lines -> the match-and-extract path -> the
 * ordering.  out (out_cap bytes) receives the delivered lines' original bytes one behind the other, each with its terminator as the text
 * has it; out_offsets (optional, lines_out + 1 entries, uint32 whatever opts->offsets64 says: the text is below 4 GiB) delimits them -- a
 * last line of the text without a terminator is copied as it is and may now lie in the middle, so the output is cut at out_offsets, not
 * at line ends.  out_index, out_values and out_class (optional, lines_out entries each) hold line numbers of the text, the numbers and
 * the classes.  All are sized by the size query (all five NULL); *n_lines entries (+ 1) always suffice.  counts (optional,
 * uint64_t[2K + 2], host) and *n_lines (optional) as gx_text_top_lines delivers them.  Limits and options are gx_text_top_lines'.  Like
 * every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_sort_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_top_part* parts, uint32_t n_parts,
                       const gx_where_term* terms, uint32_t n_terms, uint32_t flags, uint8_t* out, uint64_t out_cap, void* out_offsets,
                       uint32_t* out_index, int64_t* out_values, uint8_t* out_class, gx_sort_totals* totals, uint64_t* counts,
                       uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- Lines grouped by TWO captured texts, on the device (gx_group_pairs) ----
 * The reference's caller keys on two captured texts at once right behind the extraction (README.md:26,63-79):
 *     r = gorp.extract(line);
 *     if (r != null) seen.computeIfAbsent(r.asMap().get("verb"), v -> new HashSet<>()).add(r.asMap().get("path"));   // distinct paths per verb
 *     if (r != null) byBoth.merge(List.of(r.asMap().get("verb"), r.asMap().get("path")), 1L, Long::sum);              // lines per (verb, path)
 * -- COUNT(DISTINCT b) GROUP BY a and GROUP BY a, b.  Neither is a gx_group_lines call: it keys on one group, and two values one
 * behind the other are no key (("ab","c") and ("a","bc") differ).
 * PARTS: gx_group_lines' parts, plus second_groups[n_parts]: per part the group whose value is the line's SECOND, in
 * [0, gx_num_groups(h, extraction)), or -1: the part's lines have a key and no second.
 * THE RULE: a line counts, is keyed or adds to `unset` exactly as in gx_group_lines; nothing of that call is reinterpreted.  A keyed line
 * is PAIRED when its part's second group is >= 0 and that group's capture names a value (the rule of gx_where_term: an unset group,
 * begin < 0 <= end, end < begin or an end beyond the line is never dereferenced); every other keyed line is UNPAIRED: keyed == paired +
 * unpaired.  The empty second is a value like any other.  Two paired lines hold the same PAIR when they have the same key and their
 * seconds have the same number of code units and the same units; the seconds of different parts live in one space, as the keys do.
 * ORDER: pairs leave ordered by the first input line that holds them (pair_first_line ascends).
 * EXACT: every output is exact and the same bits on every run; all merges are unsigned integer adds and maxima.
 * NOT IN SCOPE: stats per pair, quantiles per pair, ranking pairs, more than two texts. */
typedef struct gx_pairs_out {      /* every pointer optional; device memory with opts->device_pointers, else host */
    void*     pair_units;          /* the pairs' SECOND values, one behind the other, in the batch's code units */
    uint64_t  pair_units_cap;      /* in code units */
    void*     pair_offsets;        /* n_pairs + 1, uint32 or uint64 as opts->offsets64 */
    uint32_t* pair_key;            /* the key number (gx_group_out's order) of pair p */
    uint32_t* pair_first_line;     /* pairs are ORDERED by it */
    uint64_t* pair_lines;
    uint64_t* key_pairs;           /* per KEY: its distinct seconds = its pairs; capacity keys->max_keys (keys == NULL: 0) */
    uint32_t* line_pair;           /* n entries, 0xFFFFFFFF: none */
    uint64_t  max_pairs;           /* capacity of the per-pair arrays, and the pair table's size; read in the size query too; <= 2^30 */
} gx_pairs_out;

typedef struct gx_pairs_totals {   /* host, always */
    gx_group_totals group;         /* exactly what gx_group_lines reports for the same call */
    uint64_t n_pairs, pair_units, paired, unpaired, pairs_exact;
} gx_pairs_totals;

/* gx_group_pairs: everything gx_group_lines delivers through `keys` and totals->group is delivered bit for bit, and the batch is read
 * exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging or device_pointers; the
 * stream; GX_GROUP_WEAK_HASH applies to both tables).  With pairs == NULL the call IS gx_group_lines: the pair passes do not run, and the
 * pair totals are zero with pairs_exact = 1.
 * THE PAIR TABLE has the smallest power of two >= max(64, 2 * max_pairs) slots; the number of lines is always a sufficient max_pairs.
 * HOST WAITS: ONE host wait before any output -- the wait in which gx_group_lines reads its totals also reads n_pairs, pair_units,
 * paired, unpaired and the pair table's state, computed behind the build on the same stream.  With host outputs a second wait delivers
 * them.  With device_pointers the emits are left running on opts->stream when the call returns, as gx_group_lines leaves its emit; the
 * handle's next group call on another stream waits for them, and the batch must stay unchanged until they have run.
 * SIZE QUERY: every output of `keys` and `pairs` NULL: only *totals is filled; keys->max_keys and pairs->max_pairs are still read as
 * the tables' sizes.
 * GX_E_LIMIT: a per-pair array (pair_offsets, pair_key, pair_first_line, pair_lines) with n_pairs > max_pairs; pair_units with
 * pair_units > pair_units_cap; key_pairs with n_keys > keys->max_keys; pair_offsets without offsets64 and 4 G units or more; max_pairs >
 * 2^30; a full pair table (pairs_exact = 0 and n_pairs = slots + 1, while group.exact stays 1); and gx_group_lines' own limits.  In
 * every one of these cases nothing is written to ANY output, the key outputs included, and *totals is filled (after the overflow of
 * the KEY table the pair totals are zero).
 * GX_E_ARG: every refusal gx_group_lines makes; second_groups == NULL with n_parts > 0; a second group that is neither -1 nor one of
 * its part's extraction's; an output of `pairs` given while n_parts > 0 and every second group is -1 (there is nothing they could
 * hold: ask gx_group_lines).  All refusals that need no device come before the device is looked at: a host-only handle gives them, and
 * GX_E_DEVICE after them (there is no CPU path).  n == 0 and n_parts == 0 are legal and give all zeros (pair_offsets: its one entry;
 * line_pair: all none).
 * The device workspace stays on the handle beside gx_group_lines', two buffers of their own: 28 bytes per pair slot plus 8 per key slot,
 * and 25 bytes per input line plus 16 per 2 048 lines, until gx_destroy. */
int gx_group_pairs(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                   const gx_group_part* parts, uint32_t n_parts, const int32_t* second_groups, const gx_where_term* terms, uint32_t n_terms,
                   uint32_t flags, const gx_group_out* keys, const gx_pairs_out* pairs, gx_pairs_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the pairs at its end: raw text -> lines -> the match-and-extract path -> the keys
 * and the pairs.  counts and *n_lines as gx_text_group_lines delivers them; line_pair holds one entry per line of the text.  Like every
 * gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_pairs(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                        const int32_t* second_groups, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys,
                        const gx_pairs_out* pairs, gx_pairs_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- Lines counted and measured per interval of a captured number, on the device (gx_bucket_lines) ----
 * The reference's caller asks of a timestamp "how many per minute, and how slow were they, minute by minute" right behind the
 * extraction (README.md:26,63-79, with a timestamp field):
 *     r = gorp.extract(line);
 *     if (r != null) {
 *         long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
 *         perMinute.merge(b, 1L, Long::sum);                                            // a TreeMap: buckets in time order
 *         latency.computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
 *     }
 * -- GROUP BY floor((number - origin) / width).  It is no gx_group_lines call (that keys on the text: two timestamps a millisecond apart
 * are two keys) and no gx_capture_stats histogram (at most 64 edges, known beforehand).
 * PARTS: a part names, for the lines of one extraction, number_group -- the number that is bucketed, parsed under its gx_number_format
 * and classed exactly as gx_capture_stats classes a value -- and optionally value_group, measured per bucket as gx_group_lines measures
 * one per key (-1: count only).  At most one part per extraction, at most 64 parts; all parts share ONE bucket space.
 * WHICH LINES COUNT: a line counts when its outcome is a matched extraction that has a part and every term of that extraction holds
 * (gx_capture_stats' rule).  A line that counts is BUCKETED, or its number group is UNSET, or its value is NO NUMBER, or its bucket is
 * OUT OF RANGE: lines == bucketed + unset + not_numbers + out_of_range.
 * THE BUCKET: b = floor((v - origin) / width), exact for every int64 v and origin and every width >= 1 (the 65-bit difference is taken
 * exactly).  A bucket outside [INT64_MIN + 1, INT64_MAX] is out of range and the line has no bucket.  This differs from Java on purpose:
 * Math.subtractExact would throw where v - origin overflows, while here the difference is exact and only the bucket number is limited.
 * Only the bucket NUMBER is delivered, never origin + b * width, which can overflow.
 * ORDER: buckets leave in ascending order of their number.  Only occupied buckets are delivered; an empty interval has no entry.
 * EXACT: every output is exact and the same bits on every run; all merges are unsigned integer adds and maxima.
 * NOT IN SCOPE: a text key beside the bucket (a series per verb), empty buckets filled in, calendar widths (months, local days),
 * quantiles per bucket.  The rule: gorp_amd/csrc/gx_bucket.hpp. */
#define GX_BUCKET_ALL_DIGITS 2u   /* test hook beside GX_GROUP_WEAK_HASH (1u): sort all 11 digits whatever the buckets' range is */

typedef struct gx_bucket_part {    /* the lines of ONE extraction: which group is the number, which (if any) is measured */
    int32_t extraction;            /* k in [0, K); at most one part per extraction */
    int32_t number_group;          /* g in [0, gx_num_groups(h, k)) */
    int32_t value_group;           /* -1: count only; else a group parsed as gx_capture_stats parses one */
    uint32_t reserved;             /* 0 */
} gx_bucket_part;

typedef struct gx_bucket_out {     /* 48 bytes; every pointer optional; device memory with opts->device_pointers, else host */
    int64_t*  bucket_number;       /* ascending */
    uint32_t* bucket_first_line;   /* the first input line in bucket j */
    uint64_t* bucket_lines;        /* lines in bucket j */
    gx_measure_stats* bucket_stats;/* per bucket, over its lines whose part has a value_group (exact 128-bit sum; no histogram) */
    uint32_t* line_bucket;         /* n entries: the index j of every input line's bucket, 0xFFFFFFFF for a line that has none */
    uint64_t  max_buckets;         /* capacity of the four per-bucket arrays, and the table's size; read in the size query too; <= 2^30 */
} gx_bucket_out;

typedef struct gx_bucket_totals {  /* 72 bytes; host, always */
    uint64_t n_buckets;            /* what the outputs need */
    uint64_t lines;                /* lines that count */
    uint64_t bucketed, unset, not_numbers, out_of_range;   /* lines == bucketed + unset + not_numbers + out_of_range */
    uint64_t exact;                /* 1: n_buckets is exact; 0: the table overflowed, n_buckets is only a lower bound */
    int64_t  first_bucket, last_bucket;   /* the smallest and the largest bucket number; 0 when there is no bucket */
} gx_bucket_totals;

/* gx_bucket_lines: the batch bytes / offsets / n / ids / caps is read exactly as gx_group_lines reads it (row formats int32 + dense, u16
 * and u8; offsets64; utf16; utf8 = 1; staging or device_pointers; the stream).  The buckets are found in a hash table on the device of
 * the smallest power of two >= max(64, 2 * max_buckets) slots of one 64-bit word each.
 * SIZE QUERY: every output pointer NULL (or out == NULL): only *totals is delivered, and max_buckets is still read, as the table's size.
 * GX_E_LIMIT: a per-bucket array given and n_buckets > max_buckets -- nothing is written to any output and *totals is filled; a line that
 * finds no free slot -- exact = 0 and n_buckets = slots + 1 (the number of lines is always a sufficient max_buckets); max_buckets above
 * 2^30; more than 64 parts; n of 2^32 - 1 and more; a line of 2^32 code units and more (or offsets that go backwards).
 * GX_E_ARG: parts == NULL with n_parts > 0, totals == NULL, a part's extraction or group out of range, two parts for one extraction,
 * reserved != 0, unknown flag bits, width < 1, bucket_stats without a value_group, every refusal of a term (gx_select_lines_where),
 * parts or terms on dense ids without caps, utf8 = 2, no_sync.  All refusals that need no device come before the device is looked at: a
 * host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).  n == 0 and n_parts == 0 are legal: no buckets, all
 * zeros, line_bucket all none.
 * HOST WAITS: the call synchronises the stream once, where the host reads the totals, the number of buckets and the range of their
 * numbers (from which it plans the sort's digits); with host outputs a second wait delivers them.  With device_pointers the sort and the
 * emit are left running on opts->stream when the call returns (stream order delivers the outputs); the handle's next gx_bucket_lines
 * on another stream waits for them, and the batch must stay unchanged until they have run.
 * The device workspace stays on the handle until gx_destroy: 29 bytes per slot (93 with a value group), 4 per input line, and 24 per
 * bucket plus 768 per 2 048 buckets for the sort. */
int gx_bucket_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                    const gx_bucket_part* parts, uint32_t n_parts, int64_t origin, int64_t width, const gx_where_term* terms,
                    uint32_t n_terms, uint32_t flags, const gx_bucket_out* out, gx_bucket_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with this call at its end: raw text -> lines -> the match-and-extract path -> the
 * buckets.  counts and *n_lines as gx_text_group_lines delivers them; line_bucket holds one entry per line of the text.  Like every
 * gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_bucket_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_bucket_part* parts, uint32_t n_parts, int64_t origin,
                         int64_t width, const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_bucket_out* out,
                         gx_bucket_totals* totals, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- A series per captured text: lines counted and measured per (key, interval), on the device (gx_group_series) ----
 * The reference's caller asks the question of gx_bucket_lines per verb, per host, per path right behind the extraction
 * (README.md:26,63-79, with a timestamp field):
 *     r = gorp.extract(line);
 *     if (r != null) {
 *         long b = Math.floorDiv(Instant.parse(r.asMap().get("ts")).toEpochMilli() - origin, 60_000L);
 *         perVerb.computeIfAbsent(r.asMap().get("verb"), v -> new TreeMap<Long, Stats>())
 *                .computeIfAbsent(b, x -> new Stats()).record(Long.parseLong(r.asMap().get("timeTakenInMsec")));
 *     }
 * -- GROUP BY verb, floor((ts - origin) / width).  gx_group_lines keys on one text, gx_group_pairs on two texts (two stamps a millisecond
 * apart are two seconds), gx_bucket_lines has one bucket space for all lines.
 * PARTS: gx_group_lines' parts, plus number_groups[n_parts]: per part the group whose value is the line's NUMBER, parsed under its
 * gx_number_format, in [0, gx_num_groups(h, extraction)), or -1: the part's lines have a key and no number.  origin and width >= 1 are
 * gx_bucket_lines'.  All parts share one key space and one bucket space.
 * THE RULE: a line counts, is keyed or adds to `unset` exactly as in gx_group_lines; nothing of that call is reinterpreted.  A keyed line
 * is CELLED when its part has a number group, that group's capture names a value (the rule of gx_where_term), the value parses and
 * gx_bucket_lines' rule gives it a bucket; else it adds to number_unset (the number group is -1, or its capture names nothing), to
 * not_numbers (the value does not parse) or to out_of_range (gx_bucket_lines' rule): keyed == celled + number_unset + not_numbers +
 * out_of_range.  Lines without a key are never bucketed.  Two celled lines are in the same CELL when they hold the same key
 * (gx_group_lines' equality) and the same bucket number.
 * ORDER: cells leave ordered by (key number, bucket number): key numbers are gx_group_lines' (first appearance), buckets ascend inside a
 * key, and every key's cells are contiguous -- a series per key, in time order.  The distinct bucket numbers that hold at least one cell
 * leave ascending, as an axis (bucket_number), and a cell names its bucket by its index into that axis: a dense key x time matrix needs
 * no search.
 * EXACT: every output is exact and the same bits on every run; all merges are unsigned integer adds and maxima.
 * NOT IN SCOPE: empty cells filled in, calendar widths, quantiles per cell, ranking cells, lines per bucket across keys (that is
 * gx_bucket_lines), more than one text key (compose with gx_group_pairs later).  The rule: gorp_amd/csrc/gx_series.hpp. */
typedef struct gx_series_out {     /* every pointer optional; device memory with opts->device_pointers, else host */
    int64_t*  bucket_number;       /* the axis: distinct buckets that hold a cell, ascending */
    uint32_t* cell_key;            /* key number (gx_group_out's order) of cell c; cells are ORDERED by (cell_key, cell_bucket) */
    uint32_t* cell_bucket;         /* index into bucket_number */
    uint32_t* cell_first_line;
    uint64_t* cell_lines;
    gx_measure_stats* cell_stats;  /* over the cell's lines whose part has a value_group; NULL where no part has one */
    uint64_t* key_cell_begin;      /* n_keys + 1: key j's cells are [key_cell_begin[j], key_cell_begin[j+1]); capacity keys->max_keys + 1 */
    uint32_t* line_cell;           /* n entries, 0xFFFFFFFF: none */
    uint64_t  max_cells;           /* capacity of the per-cell arrays, and BOTH tables' size; read in the size query too; <= 2^30 */
    uint64_t  max_buckets;         /* capacity of bucket_number only */
} gx_series_out;

typedef struct gx_series_totals {  /* host, always */
    gx_group_totals group;         /* exactly what gx_group_lines reports for the same call */
    uint64_t n_cells, n_buckets, celled, number_unset, not_numbers, out_of_range, cells_exact;
    int64_t  first_bucket, last_bucket;   /* 0 without a cell */
} gx_series_totals;

/* gx_group_series: everything gx_group_lines delivers through `keys` and totals->group is delivered bit for bit.
 * HOW THE BATCH IS READ: exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging
 * or device_pointers; the stream).
 * FLAGS: GX_GROUP_WEAK_HASH (it cuts the hashes of all three tables to 3 bits) and GX_BUCKET_ALL_DIGITS (it applies to both sorts).
 * With series == NULL the call IS gx_group_lines: the series passes do not run, and the series totals are zero with cells_exact = 1.
 * Its arguments are still checked: number_groups == NULL with n_parts > 0, a bad number group and width < 1 are GX_E_ARG there too.
 * THE TABLES: a table of the distinct buckets and a table of the distinct cells, each of the smallest power of two >= max(64, 2 *
 * max_cells) slots of one 64-bit word; distinct buckets never exceed distinct cells.  The number of lines is always a sufficient
 * max_cells.
 * SIZE QUERY: every output of `keys` and `series` NULL: only *totals is filled; keys->max_keys and series->max_cells are still read as
 * the tables' sizes.
 * GX_E_LIMIT: a per-cell array (cell_key, cell_bucket, cell_first_line, cell_lines, cell_stats) with n_cells > max_cells; bucket_number
 * with n_buckets > max_buckets; key_cell_begin with n_keys > keys->max_keys; max_cells > 2^30; a full table (cells_exact = 0 and n_cells
 * = slots + 1, while group.exact stays 1); and gx_group_lines' own limits.  In every one of these cases nothing is written to ANY
 * output, the key outputs included, and *totals is filled (after the overflow of the KEY table the series totals are zero).
 * GX_E_ARG: every refusal gx_group_lines makes; number_groups == NULL with n_parts > 0; a number group that is neither -1 nor one of its
 * part's extraction's; width < 1; cell_stats where no part has a value group; an output of `series` given while n_parts > 0 and every
 * number group is -1; unknown flag bits.  All refusals that need no device come before the device is looked at: a host-only handle
 * gives them, and GX_E_DEVICE after them (there is no CPU path).
 * EMPTY INPUTS: n == 0 and n_parts == 0 are legal and give all zeros (key_cell_begin: its one entry; line_cell: all none).
 * HOST WAITS: ONE host wait before any output -- the wait in which gx_group_lines reads its totals also reads the series totals, the
 * buckets, the cells and the range of the bucket numbers, from which both sorts' digits are planned.  With host outputs a second wait
 * delivers them.  With device_pointers the sorts and the emits are left running on opts->stream when the call returns, as
 * gx_bucket_lines leaves them; the handle's next group call on another stream waits for them, and the batch must stay unchanged until
 * they have run.
 * WORKSPACE: on the handle beside gx_group_lines', until gx_destroy: 21 bytes per bucket slot and 37 per cell slot (101 with a value
 * group), 4 per input line, and 28 per cell plus 768 per 2 048 cells for the sorts. */
int gx_group_series(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                    const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups, int64_t origin, int64_t width,
                    const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_series_out* series,
                    gx_series_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the series at its end: raw text -> lines -> the match-and-extract path -> the
 * keys and the cells.  counts and *n_lines as gx_text_group_lines delivers them; line_cell holds one entry per line of the text.  Like
 * every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_series(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                         const int32_t* number_groups, int64_t origin, int64_t width, const gx_where_term* terms, uint32_t n_terms,
                         uint32_t flags, const gx_group_out* keys, const gx_series_out* series, gx_series_totals* totals, uint64_t* counts,
                         uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- Sessions per captured text: a key's lines in time order, cut where the log falls silent, on the device (gx_group_sessions) ----
 * The reference's caller collects a request's, a user's or a connection's lines right behind the extraction (README.md:26,63-79) and asks
 * which of them belong together:
 *     byId.computeIfAbsent(r.asMap().get("id"), k -> new ArrayList<>()).add(r);
 *     ... per id: sort by Instant.parse(ts).toEpochMilli(); a new session wherever ts - previous ts > maxGap
 * -- Splunk's `transaction id maxpause=30s`; SQL's SUM(CASE WHEN ts - LAG(ts) OVER (PARTITION BY id ORDER BY ts) > gap THEN 1 ELSE 0 END).
 * gx_group_series cuts time into fixed intervals from an origin: it cuts a session wherever it crosses an interval's edge and joins two
 * that share an interval.  A session depends on the ORDER of a key's lines in time.
 * PARTS: gx_group_lines' parts, plus number_groups[n_parts] exactly as gx_group_series takes them: per part the group whose value is the
 * line's TIME, parsed under its gx_number_format, in [0, gx_num_groups(h, extraction)), or -1: the part's lines have a key and no time.
 * All parts share one key space.
 * THE RULE: a line counts, is keyed or adds to `unset` exactly as in gx_group_lines; nothing of that call is reinterpreted.  A keyed line
 * is an ENTRY when its part has a number group, that group's capture names a value (the rule of gx_where_term) and the value parses
 * (gx_top_lines' class "number"); else it adds to number_unset (the number group is -1, or its capture names nothing) or to not_numbers
 * (the value does not parse): keyed == entries + number_unset + not_numbers.  Key j's entries are ordered by (time ascending, input line
 * ascending).  A SESSION begins at the key's first entry and at every entry whose time exceeds the previous entry's time by MORE than
 * max_gap (>= 0, an int64 in the number's own unit).  The comparison is exact for every pair of int64: in that order t >= prev, so
 * (uint64) t - (uint64) prev is the true difference (up to 2^64 - 1), compared unsigned with (uint64) max_gap.  Equal times never open a
 * session; max_gap = INT64_MAX still splits INT64_MIN from INT64_MAX.
 * ORDER: sessions leave ordered by (key number, begin time): key numbers are gx_group_lines' (first appearance), a key's sessions are
 * contiguous and in time order.  Entries leave ordered by (key number, time, input line): a session's entries are contiguous.
 * EXACT: every output is exact and the same bits on every run; ranks come from ballots, merges are integer adds, minima and maxima; no
 * float anywhere.
 * NOT IN SCOPE: a cap on a session's span (maxspan), start / end markers (startswith), carrying unstamped lines into a session (compose
 * with gx_sort_lines' carry later), the sessions' text as a new CSR batch (compose entry_line with the existing copy later), quantiles
 * of durations, ranking sessions.  The rule: gorp_amd/csrc/gx_sessions.hpp. */
typedef struct gx_sessions_out {      /* every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* session_key;            /* key number of session s; sessions ORDERED by (session_key, session_begin) */
    int64_t*  session_begin;          /* time of its first entry */
    int64_t*  session_end;            /* time of its last entry: duration = end - begin as uint64 */
    uint32_t* session_first_line;     /* input line of its first entry */
    uint64_t* session_lines;          /* its entries */
    gx_measure_stats* session_stats;  /* over its entries whose part has a value_group; NULL where no part has one */
    uint64_t* session_entry_begin;    /* n_sessions + 1: session s's entries are entry_line[begin[s], begin[s+1]) */
    uint64_t* key_session_begin;      /* n_keys + 1; capacity keys->max_keys + 1 */
    uint32_t* entry_line;             /* the entries' input lines in (key, time, line) order; capacity max_entries */
    uint32_t* line_session;           /* n entries, 0xFFFFFFFF: the line is no entry */
    uint64_t  max_sessions;           /* capacity of the per-session arrays (session_entry_begin: + 1); <= 2^30 */
    uint64_t  max_entries;            /* capacity of entry_line */
} gx_sessions_out;

typedef struct gx_sessions_totals {   /* host, always */
    gx_group_totals group;            /* exactly what gx_group_lines reports for the same call */
    uint64_t n_sessions, entries, number_unset, not_numbers;
    uint64_t longest_lines;           /* the most entries in one session; 0 without one */
    uint64_t longest_duration;        /* the largest end - begin, unsigned; 0 without one */
    int64_t  first_time, last_time;   /* over all entries; 0 without one */
} gx_sessions_totals;

/* gx_group_sessions: everything gx_group_lines delivers through `keys` and totals->group is delivered bit for bit.
 * HOW THE BATCH IS READ: exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging
 * or device_pointers; the stream).
 * FLAGS: GX_GROUP_WEAK_HASH and GX_BUCKET_ALL_DIGITS (both sorts take every digit: the same result, only slower).
 * With sessions == NULL the call IS gx_group_lines: the session passes do not run, and the session totals are zero.  Its arguments are
 * still checked: number_groups == NULL with n_parts > 0, a bad number group and max_gap < 0 are GX_E_ARG there too.
 * SIZE QUERY: every output of `keys` and `sessions` NULL: only *totals is filled; keys->max_keys is still read as the table's size.
 * entries is always a sufficient max_sessions and max_entries.
 * GX_E_LIMIT: a per-session array (session_key, session_begin, session_end, session_first_line, session_lines, session_stats,
 * session_entry_begin) with n_sessions > max_sessions; entry_line with entries > max_entries; key_session_begin with n_keys >
 * keys->max_keys; max_sessions > 2^30; more than 2^30 entries; and gx_group_lines' own limits.  In every one of these cases nothing is
 * written to ANY output, the key outputs included, and *totals is filled (after the overflow of the key table the session totals are
 * zero; with more than 2^30 entries n_sessions and the longest are).
 * GX_E_ARG, in this order behind every refusal gx_group_lines makes: number_groups == NULL with n_parts > 0; a number group that is
 * neither -1 nor one of its part's extraction's; max_gap < 0; session_stats where no part has a value group; an output of `sessions`
 * given while n_parts > 0 and every number group is -1; unknown flag bits are among gx_group_lines' refusals.  All refusals that need no
 * device come before the device is looked at: a host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).
 * EMPTY INPUTS: n == 0 and n_parts == 0 are legal and give all zeros (session_entry_begin and key_session_begin: their one entry;
 * line_session: all none).
 * HOST WAITS: TWO host waits before any output.  The wait in which gx_group_lines reads its totals also reads entries, number_unset,
 * not_numbers, first_time, last_time and the OR and AND of the times, from which the time sort's digits are planned.  n_sessions exists
 * only behind the two sorts: ONE more wait reads n_sessions, longest_lines and longest_duration, before the key outputs are written, so
 * that a capacity can be refused with every output untouched.  Without an entry that wait is not taken.  With host outputs a further
 * wait delivers them.  With device_pointers the emits are left running on opts->stream when the call returns; the handle's next group
 * call on another stream waits for them, and the batch must stay unchanged until they have run.
 * WORKSPACE: on the handle beside gx_group_lines', until gx_destroy: 17 bytes per input line (26 with a value group); 65 bytes per entry
 * and 1 536 per 2 048 entries for the sorts, the heads and the sessions; with session_stats 80 more per entry. */
int gx_group_sessions(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                      const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups, int64_t max_gap,
                      const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_sessions_out* sessions,
                      gx_sessions_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the sessions at its end: raw text -> lines -> the match-and-extract path -> the
 * keys and the sessions.  counts and *n_lines as gx_text_group_lines delivers them; line_session holds one entry per line of the text.
 * Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_sessions(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                           const int32_t* number_groups, int64_t max_gap, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                           const gx_group_out* keys, const gx_sessions_out* sessions, gx_sessions_totals* totals, uint64_t* counts,
                           uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- Begin/end spans per captured text: a key's start and end lines paired in input order, on the device (gx_group_spans) ----
 * An application logs one line when work starts and another when it ends; two extractions capture the same id.  The reference's caller
 * pairs them right behind the extraction:
 *     r = gorp.extract(line);
 *     if (r != null && r.name().equals("RequestStart")) { prev = open.put(id(r), r); if (prev != null) superseded.add(prev); }
 *     if (r != null && r.name().equals("RequestEnd"))   { b = open.remove(id(r)); if (b == null) orphanEnds.add(r); else took.record(ts(r) - ts(b)); }
 *     ... at the end: open.values() are the requests that started and never finished
 * -- Splunk's `transaction id startswith=... endswith=...`.
 * PARTS: gx_group_lines' parts, plus number_groups[n_parts] exactly as gx_group_sessions takes them (per part the group whose value is
 * the line's TIME, parsed under its gx_number_format, in [0, gx_num_groups(h, extraction)), or -1), plus roles[n_parts]: per part
 * GX_SPAN_BEGIN or GX_SPAN_END.  All parts share one key space.
 * THE RULE: a line counts, is keyed or adds to `unset` exactly as in gx_group_lines; nothing of that call is reinterpreted.  Every keyed
 * line is an ENTRY, and its role is its part's.  A key's entries are taken in INPUT order; time plays no part in pairing, which works
 * with every number group -1.  An END entry forms a SPAN with the entry immediately before it among its key's entries if and only if that
 * entry is a BEGIN.  This equals the put / remove loop above for every input, because put replaces and remove empties.  Every entry has
 * one STATE: 1 a span's begin; 2 a span's end; 3 a BEGIN superseded (the next entry of its key is another BEGIN); 4 a BEGIN left open (it
 * is its key's last entry); 5 an END without a begin (it is its key's first entry, or follows an END); 0: the line is no entry.
 * DURATION: each side's time is classed as gx_top_lines classes a value -- 0 number, 1 unset (the number group is -1, or its capture
 * names nothing), 2 not a number (the value does not parse); the span's class is the larger of the two.  With both sides numbers,
 * duration = end - begin exactly: the difference is taken in uint64 and the order of the two times decides whether it lies in int64.  A
 * duration outside int64 makes the span class 2 and adds to out_of_range; a negative duration (the end stamped earlier than the begin) is
 * a number like any other.  span_begin, span_end and span_duration are 0 where they are not numbers.
 * ORDER: spans leave ordered by (key number, input line of the end): key numbers are gx_group_lines' (first appearance), a key's spans
 * are contiguous.
 * IDENTITIES: keyed == begins + ends; begins == n_spans + superseded + left_open; ends == n_spans + orphan_ends; durations.lines ==
 * n_spans; out_of_range <= durations.not_numbers.
 * EXACT: every output is exact and the same bits on every run; ranks come from ballots, merges are integer adds, minima and maxima; no
 * float anywhere.
 * NOT IN SCOPE: pairing in time order, roles chosen by a captured value instead of by extraction, nested or re-entrant spans (a depth
 * counter), carrying open begins into the next batch (key_open_line is what a caller needs for that), the spans' text as a CSR batch,
 * quantiles of durations, ranking spans.  The rule: gorp_amd/csrc/gx_spans.hpp. */
#define GX_SPAN_BEGIN 1u
#define GX_SPAN_END   2u
typedef struct gx_spans_out {         /* every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* span_key;               /* key number of span s; spans ORDERED by (span_key, span_end_line) */
    uint32_t* span_begin_line;        /* input lines of the two sides */
    uint32_t* span_end_line;
    int64_t*  span_begin;             /* their times; 0 where the side's class is not 0 */
    int64_t*  span_end;
    int64_t*  span_duration;          /* end - begin where span_class is 0, else 0 */
    uint8_t*  span_class;             /* 0 duration, 1 unset, 2 not a number (out of range included) */
    uint64_t* key_span_begin;         /* n_keys + 1; capacity keys->max_keys + 1 */
    gx_measure_stats* key_span_stats; /* per key over its spans' durations: lines = spans, numbers / unset / not_numbers by span_class, min,
                                         max, exact 128-bit sum; capacity keys->max_keys */
    uint32_t* key_open_line;          /* per key: the BEGIN line left open at the end of the batch, 0xFFFFFFFF: none; capacity keys->max_keys */
    uint32_t* line_span;              /* n entries: the span a line begins or ends, 0xFFFFFFFF otherwise */
    uint8_t*  line_state;             /* n entries: 0 .. 5 as above */
    uint64_t  max_spans;              /* capacity of the per-span arrays; <= 2^30 */
} gx_spans_out;

typedef struct gx_spans_totals {      /* host, always */
    gx_group_totals group;            /* exactly what gx_group_lines reports for the same call */
    uint64_t n_spans, begins, ends, superseded, left_open, orphan_ends, out_of_range;
    gx_measure_stats durations;       /* over all spans, as key_span_stats is per key */
} gx_spans_totals;

/* gx_group_spans: everything gx_group_lines delivers through `keys` and totals->group is delivered bit for bit.
 * HOW THE BATCH IS READ: exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging
 * or device_pointers; the stream).
 * FLAGS: GX_GROUP_WEAK_HASH and GX_BY_KEY_ALL_DIGITS (the sort takes every digit: the same result, only slower).
 * With spans == NULL the call IS gx_group_lines: the span passes do not run, and the span totals are zero.  Its arguments are still
 * checked: number_groups == NULL or roles == NULL with n_parts > 0, a bad number group and a bad role are GX_E_ARG there too.
 * SIZE QUERY: every output of `keys` and `spans` NULL: only *totals is filled; keys->max_keys is still read as the table's size.
 * group.keyed / 2 is always a sufficient max_spans.
 * GX_E_LIMIT: a per-span array (span_key, span_begin_line, span_end_line, span_begin, span_end, span_duration, span_class) with n_spans >
 * max_spans; key_span_begin, key_span_stats or key_open_line with n_keys > keys->max_keys; max_spans > 2^30; more than 2^30 entries; and
 * gx_group_lines' own limits.  In every one of these cases nothing is written to ANY output, the key outputs included, and *totals is
 * filled (after the overflow of the key table and with more than 2^30 entries the span totals are zero).
 * GX_E_ARG, in this order behind every refusal gx_group_lines makes: number_groups == NULL with n_parts > 0; a number group that is
 * neither -1 nor one of its part's extraction's; roles == NULL with n_parts > 0; a role that is neither GX_SPAN_BEGIN nor GX_SPAN_END;
 * unknown flag bits are among gx_group_lines' refusals.  Outputs of durations are legal when every number group is -1: every span is
 * then class 1.  All refusals that need no device come before the device is looked at: a host-only handle gives them, and GX_E_DEVICE
 * after them (there is no CPU path).
 * EMPTY INPUTS: n == 0 and n_parts == 0 are legal and give all zeros (key_span_begin: its one entry; line_span: all none; line_state: all
 * 0).
 * HOST WAITS: TWO host waits before any output.  The wait in which gx_group_lines reads its totals also reads the entries.  n_spans
 * exists only behind the sort: ONE more wait reads n_spans, the states' counts and totals->durations, before the key outputs are written,
 * so that a capacity can be refused with every output untouched.  Without an entry that wait is not taken.  With host outputs a further
 * wait delivers them.  With device_pointers the emits are left running on opts->stream when the call returns; the handle's next group
 * call on another stream waits for them, and the batch must stay unchanged until they have run.
 * WORKSPACE: on the handle beside gx_group_lines', until gx_destroy: 18 bytes per input line; 98 bytes per entry and 768 per 2 048
 * entries for the sort, the states and the durations' columns; 16 bytes per key; nothing per span. */
int gx_group_spans(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                   const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups, const uint32_t* roles,
                   const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_spans_out* spans,
                   gx_spans_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the spans at its end: raw text -> lines -> the match-and-extract path -> the keys
 * and the spans.  counts and *n_lines as gx_text_group_lines delivers them; line_span and line_state hold one entry per line of the text.
 * Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_spans(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                        const int32_t* number_groups, const uint32_t* roles, const gx_where_term* terms, uint32_t n_terms, uint32_t flags,
                        const gx_group_out* keys, const gx_spans_out* spans, gx_spans_totals* totals, uint64_t* counts, uint64_t* n_lines,
                        const gx_batch_opts* opts);

/* ---- Trailing time windows per captured text: a key's lines within the last W before each of them, on the device (gx_group_windows) ----
 * The question most log alerts ask -- five failed logins of one user within 60 s; more than 100 requests of one client within a second.
 * The reference's caller keeps a deque per key right behind the extraction:
 *     Deque<Long> q = recent.computeIfAbsent(r.asMap().get("user"), k -> new ArrayDeque<>());
 *     q.addLast(t);  while (t - q.peekFirst() > window) q.removeFirst();
 *     if (q.size() >= threshold && !tripped.contains(user)) alert(...)
 * -- Splunk's `streamstats time_window=60s count by user`; SQL's COUNT(*) OVER (PARTITION BY user ORDER BY ts RANGE BETWEEN 60000
 * PRECEDING AND CURRENT ROW); fail2ban's findtime and maxretry.  gx_group_series splits a burst that straddles an interval's edge;
 * gx_group_sessions chains lines that are each close to the next.  A sliding window depends on every entry's own place in its key's
 * time order.
 * PARTS: gx_group_lines' parts, plus number_groups[n_parts] exactly as gx_group_sessions takes them.  All parts share one key space.
 * THE RULE: a line counts, is keyed or adds to `unset` exactly as in gx_group_lines; a keyed line is an ENTRY exactly as in
 * gx_group_sessions: keyed == entries + number_unset + not_numbers.  Key j's entries are ordered by (time ascending, input line
 * ascending).  window is an int64 >= 0 in the time's own unit.  Entry e's WINDOW is the entries f of the same key with f <= e in that
 * order and time(e) - time(f) <= window.  The comparison is exact for every pair of int64: f <= e gives time(f) <= time(e), so (uint64)
 * time(e) - (uint64) time(f) is the true difference, compared unsigned with (uint64) window; window = INT64_MAX still keeps INT64_MIN out
 * of INT64_MAX's window; window = 0 is the entries of the same time up to e.  An entry of the same time and a later input line is NOT in
 * e's window (the caller's loop has not seen it yet).  The window is the contiguous run of entries [e - window_lines + 1, e];
 * window_lines >= 1.
 * TRIPS: threshold is a uint32, 0: no trips.  Entry e TRIPS when window_lines(e) >= threshold and e is its key's first entry or
 * window_lines(e - 1) < threshold: the edge, not the level.  A key trips again after its count fell below the threshold.  With
 * threshold 1 exactly the first entry of every key that has entries trips.
 * PEAK: a key's peak is the largest window_lines among its entries, its peak_line the input line of the FIRST entry in the order that
 * attains it; the totals' peak is the same over all entries (ties: the smallest entry index).
 * WINDOW SUMS: where a part has a value_group, an entry's window sum is over the window's entries whose value parsed: their count and
 * the exact 128-bit sum.
 * ORDER: entries and trips leave ordered by (key number, time, input line): key numbers are gx_group_lines' (first appearance).
 * EXACT: every output is exact and the same bits on every run; ranks come from ballots, merges are integer adds and maxima; no float
 * anywhere.
 * NOT IN SCOPE: windows by number of entries (streamstats window=N), centred or leading windows, window min / max / quantiles, a trip's
 * lines as a new CSR batch, windows over all keys together, state carried from one batch into the next.  The rule:
 * gorp_amd/csrc/gx_windows.hpp. */
typedef struct gx_window_sum {
    uint64_t numbers;                 /* the window's entries whose value parsed */
    uint64_t sum_lo;                  /* their exact sum: sum_hi * 2^64 + sum_lo, two's complement */
    int64_t  sum_hi;
    uint64_t reserved;                /* 0 */
} gx_window_sum;

typedef struct gx_windows_out {       /* every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* entry_line;             /* [entries] input lines in (key, time, line) order */
    uint32_t* entry_key;              /* [entries] */
    int64_t*  entry_time;             /* [entries] */
    uint32_t* entry_window_lines;     /* [entries] >= 1; entry e's window is entries [e - lines + 1, e] */
    gx_window_sum* entry_window_sum;  /* [entries]; NULL where no part has a value_group */
    uint64_t* key_entry_begin;        /* n_keys + 1; capacity keys->max_keys + 1 */
    uint32_t* key_peak_lines;         /* n_keys; 0: the key has no entry */
    uint32_t* key_peak_line;          /* n_keys; 0xFFFFFFFF: none */
    uint32_t* line_window_lines;      /* n: 0 for a line that is no entry */
    uint32_t* trip_key;               /* [n_trips] trips ORDERED by (key number, time, line) */
    uint32_t* trip_line;              /* [n_trips] input line of the entry that tripped */
    int64_t*  trip_time;              /* [n_trips] */
    uint32_t* trip_entry;             /* [n_trips] its index among the entries */
    uint64_t* key_trip_begin;         /* n_keys + 1; capacity keys->max_keys + 1 */
    uint64_t  max_entries;            /* capacity of the per-entry arrays; <= 2^30 */
    uint64_t  max_trips;              /* capacity of the per-trip arrays; <= 2^30 */
} gx_windows_out;

typedef struct gx_windows_totals {    /* host, always */
    gx_group_totals group;            /* exactly what gx_group_lines reports for the same call */
    uint64_t entries, number_unset, not_numbers;
    uint64_t n_trips, tripped_keys;   /* tripped_keys: the keys with at least one trip */
    uint64_t peak_lines;              /* the largest window_lines; 0 without an entry */
    uint32_t peak_line, peak_key;     /* input line and key number of the first entry that attains it; 0xFFFFFFFF without an entry */
    int64_t  first_time, last_time;   /* over all entries; 0 without one */
} gx_windows_totals;

/* gx_group_windows: everything gx_group_lines delivers through `keys` and totals->group is delivered bit for bit.
 * HOW THE BATCH IS READ: exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging
 * or device_pointers; the stream).
 * FLAGS: GX_GROUP_WEAK_HASH and GX_BUCKET_ALL_DIGITS (both sorts take every digit: the same result, only slower).
 * With windows == NULL the call IS gx_group_lines: the window passes do not run, and the window totals are zero (the peak's line and
 * key: 0xFFFFFFFF).  Its arguments are still checked: number_groups == NULL with n_parts > 0, a bad number group and window < 0 are
 * GX_E_ARG there too.
 * SIZE QUERY: every output of `keys` and `windows` NULL: only *totals is filled; keys->max_keys is still read as the table's size.
 * entries is always a sufficient max_entries and max_trips.
 * GX_E_LIMIT: a per-entry array (entry_line, entry_key, entry_time, entry_window_lines, entry_window_sum) with entries > max_entries; a
 * per-trip array (trip_key, trip_line, trip_time, trip_entry) with n_trips > max_trips; a per-key array (key_entry_begin,
 * key_peak_lines, key_peak_line, key_trip_begin) with n_keys > keys->max_keys; max_entries or max_trips > 2^30; more than 2^30 entries;
 * and gx_group_lines' own limits.  In every one of these cases nothing is written to ANY output, the key outputs included, and *totals
 * is filled (after the overflow of the key table the window totals are zero; with more than 2^30 entries the trips and the peak are;
 * with a capacity above 2^30 all of *totals is, since that refusal comes before the device is looked at).
 * GX_E_ARG, in this order behind every refusal gx_group_lines makes: number_groups == NULL with n_parts > 0; a number group that is
 * neither -1 nor one of its part's extraction's; window < 0; entry_window_sum where no part has a value group; a trip output
 * (trip_key, trip_line, trip_time, trip_entry, key_trip_begin) with threshold == 0; an output of `windows` given while n_parts > 0 and
 * every number group is -1; unknown flag bits are among gx_group_lines' refusals.  All refusals that need no device come before the
 * device is looked at: a host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).
 * EMPTY INPUTS: n == 0 and n_parts == 0 are legal and give all zeros (key_entry_begin and key_trip_begin: their one entry;
 * line_window_lines: all 0).
 * HOST WAITS: TWO host waits before any output.  The wait in which gx_group_lines reads its totals also reads entries, number_unset,
 * not_numbers, first_time, last_time and the OR and AND of the times, from which the time sort's digits are planned.  The trips exist
 * only behind the two sorts and the window pass: ONE more wait reads n_trips, tripped_keys and the peak, before the key outputs are
 * written, so that a capacity can be refused with every output untouched.  Without an entry that wait is not taken.  With host outputs
 * a further wait delivers them.  With device_pointers the emits are left running on opts->stream when the call returns; the handle's
 * next group call on another stream waits for them, and the batch must stay unchanged until they have run.
 * WORKSPACE: on the handle beside gx_group_lines', until gx_destroy: 17 bytes per input line (26 with a value group), shared with
 * gx_group_sessions; 73 bytes per entry and 1 536 per 2 048 entries for the sorts, the window pass and the trips; 8 bytes per key; with
 * entry_window_sum 64 more per entry. */
int gx_group_windows(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                     const gx_group_part* parts, uint32_t n_parts, const int32_t* number_groups, int64_t window, uint32_t threshold,
                     const gx_where_term* terms, uint32_t n_terms, uint32_t flags, const gx_group_out* keys, const gx_windows_out* windows,
                     gx_windows_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the windows at its end: raw text -> lines -> the match-and-extract path -> the
 * keys and the windows.  counts and *n_lines as gx_text_group_lines delivers them; line_window_lines holds one entry per line of the
 * text.  Like every gx_text_* call it returns with all its work on opts->stream done. */
int gx_text_group_windows(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                          const int32_t* number_groups, int64_t window, uint32_t threshold, const gx_where_term* terms, uint32_t n_terms,
                          uint32_t flags, const gx_group_out* keys, const gx_windows_out* windows, gx_windows_totals* totals, uint64_t* counts,
                          uint64_t* n_lines, const gx_batch_opts* opts);

/* ---- Captured texts looked up in a dictionary of the caller's, on the device.  The reference's caller does this right behind the
 * extraction, against a set or a map that it holds from elsewhere (README.md:26,63-79):
 *     if (r != null && wanted.contains(r.asMap().get("user"))) ...        meta = byHost.get(r.asMap().get("host"));
 * membership ("the requests of these 40 000 customers", "drop every line whose client ip is on the blocklist"), enrichment (the row of
 * the line's value in a dimension table) and ONE key space across batches (the keys that gx_group_lines left for batch A, looked up
 * for batch B).
 * THE DICTIONARY is n_entries texts, 0 <= n_entries <= 2^30, as a CSR: entry j is entry_units[entry_offsets[j], entry_offsets[j + 1])
 * in the batch's own code units (bytes; 16-bit units with opts->utf16; UTF-8 bytes with utf8 = 1); entry_offsets holds n_entries + 1
 * offsets, uint32 or uint64 as opts->offsets64 says, and entry_offsets[0] need not be 0 -- exactly how gx_group_out.key_units and
 * key_offsets leave.  With device_pointers both arrays lie on the device, else they are host memory and staged.  The empty entry is an
 * entry like any other.  Two entries with the same units are DUPLICATES and the lowest entry number stands for them all
 * (index.putIfAbsent(entry[j], j) for ascending j): entry_same[j] is that number, j itself for the first entry with a text.
 * PARTS are gx_group_part as they are (extraction, key_group, optional value_group; at most one part per extraction; all parts share the
 * ONE dictionary), TERMS gx_where_term as they are; "a line counts", the key's pair, its set-or-unset test (a pair that names no value
 * is never dereferenced) and key equality (the same number of units and the same units) are gx_group_lines' word for word.  A line that
 * counts is exactly one of: UNSET (its key pair names no value), a HIT (its key is some entry's text) or a MISS (the pair is set and no
 * entry has its text; every keyed line when n_entries == 0).  lines == keyed + unset, keyed == hits + misses.
 * Every output is exact and the same bits on every run.  GX_GROUP_WEAK_HASH is accepted as the same test hook: identical results. */
#define GX_LOOKUP_NONE 0xFFFFFFFFu   /* line_entry: the line does not count, or its key pair names no value */
#define GX_LOOKUP_MISS 0xFFFFFFFEu   /* line_entry: the line's key is set and is no entry */
enum { GX_LOOKUP_KEEP_NOTHING = 0, GX_LOOKUP_KEEP_HITS = 1, GX_LOOKUP_KEEP_OTHERS = 2 };

typedef struct gx_lookup_out {       /* 96 bytes; every pointer optional; device memory with opts->device_pointers, else host */
    uint32_t* line_entry;            /* n: entry_same of the entry the line's key equals, else GX_LOOKUP_MISS / GX_LOOKUP_NONE */
    uint32_t* entry_same;            /* m: the lowest entry with entry j's text */
    uint64_t* entry_lines;           /* m: lines that hit entry j; 0 where entry_same[j] != j */
    uint32_t* entry_first_line;      /* m: the first input line that hits entry j, 0xFFFFFFFF: none */
    gx_measure_stats* entry_stats;   /* m: over entry j's lines whose part has a value_group (gx_group_out.key_stats' rule) */
    uint32_t* out_index;             /* with keep != 0: the kept lines as a new CSR batch, gx_select_lines_where's five outputs */
    void*     out_bytes;
    void*     out_offsets;
    void*     out_ids;
    int32_t*  out_caps;
    uint64_t  cap_lines, out_bytes_cap;   /* as in gx_by_key_out: lines; BYTES */
} gx_lookup_out;

typedef struct gx_lookup_totals {    /* 80 bytes; host, always */
    uint64_t entries, distinct_entries, hit_entries;   /* m; entries with entry_same[j] == j; ... of those with at least one line */
    uint64_t lines, keyed, unset, hits, misses;
    uint64_t lines_out, units_out;   /* what keep keeps; 0 with GX_LOOKUP_KEEP_NOTHING */
} gx_lookup_totals;

/* gx_lookup_lines.
 * HOW THE BATCH IS READ: exactly as gx_group_lines reads it (row formats int32 + dense, u16 and u8; offsets64; utf16; utf8 = 1; staging
 * or device_pointers; the stream).
 * KEEP: GX_LOOKUP_KEEP_HITS keeps the lines that count and hit (wanted.contains(v)); GX_LOOKUP_KEEP_OTHERS keeps the lines that count
 * and do not hit, misses and unset alike (!blocked.contains(v), v == null included).  Lines that do not count are never kept.  Kept lines
 * leave in input order, copied as gx_select_lines copies one: out_index, out_bytes, out_offsets (the width of the input's), out_ids and
 * out_caps in the input's row format -- an ordinary batch for every other call.  With GX_LOOKUP_KEEP_NOTHING the five must be NULL.
 * entry_stats: gx_group_out.key_stats' rule (lines == numbers + unset + not_numbers; min and max INT64_MAX and INT64_MIN without a
 * number; the 128-bit sum exact; the parts' number formats honoured); an entry with entry_same[j] != j has the stats of nothing.
 * SIZE QUERY: out == NULL or every pointer NULL: only *totals is filled.  n is always a sufficient cap_lines.
 * GX_E_LIMIT with nothing written to any output and *totals filled: cap_lines < lines_out with a per-line batch output; out_bytes_cap
 * too small; 32-bit out_offsets with 2^32 units and more.  GX_E_LIMIT before the device is looked at: n_entries > 2^30; n >= 2^32 - 1;
 * more than 64 parts or terms.  GX_E_LIMIT from the offsets: a line or an entry of 2^32 units and more, or offsets that go backwards --
 * found on the host for host offsets, with device_pointers by the pass that reads them.
 * GX_E_ARG, in this order: h, offsets or (n > 0) ids NULL; every refusal gx_group_lines makes of totals == NULL, flags, parts, utf8 = 2,
 * terms and no_sync; entry_stats where no part has a value_group; keep > 2; a batch output with GX_LOOKUP_KEEP_NOTHING; out_caps on
 * compact rows; entry_offsets == NULL with n_entries > 0; [the limits above]; parts or terms on dense ids without caps; out_caps
 * without caps; entry_units == NULL where host offsets name a unit; an output that overlaps an input or the dictionary.  All of these
 * come before the device is looked at: a host-only handle gives them, and GX_E_DEVICE after them (there is no CPU path).
 * EMPTY INPUTS: n == 0, n_parts == 0 and n_entries == 0 are legal (entry_same is delivered whatever the lines are).
 * HOST WAITS: ONE wait, in which the host reads the totals, lines_out and units_out among them (gx_select.hip's scans run behind the
 * probe on the same stream).  With host outputs a second wait delivers them.  With device_pointers the emit and the copy are left
 * running on opts->stream when the call returns; the handle's next call on another stream waits for them, and the batch and the
 * dictionary must stay unchanged until they have run.
 * WORKSPACE: on the handle until gx_destroy: two to four table slots per entry (64 at least) of 32 bytes each, 96 with a value group;
 * 4 bytes per entry; 4 per line; with keep gx_select_lines' 21 per line. */
int gx_lookup_lines(gx_handle* h, const void* bytes, const void* offsets, uint64_t n, const void* ids, const int32_t* caps,
                    const gx_group_part* parts, uint32_t n_parts, const gx_where_term* terms, uint32_t n_terms,
                    const void* entry_units, const void* entry_offsets, uint64_t n_entries, uint32_t keep, uint32_t flags,
                    const gx_lookup_out* out, gx_lookup_totals* totals, const gx_batch_opts* opts);

/* The whole-file form, gx_text_group_lines' chain with the lookup at its end: raw text -> lines -> the match-and-extract path -> the
 * lookup.  `out` carries the per-line and per-entry arrays only (its five batch pointers must be NULL: GX_E_ARG); line_entry holds one
 * entry per line of the text.  kept, kept_offsets and kept_index are gx_text_lines_by_key's out, out_offsets and out_index -- the kept
 * lines' original bytes one after the other, terminators included, as gx_text_select writes them (kept_cap BYTES; units_out counts
 * them), their lines + 1 offsets (32-bit) and their line numbers in the text -- sized by the size query (all three NULL:
 * totals->lines_out and units_out); they must be NULL with GX_LOOKUP_KEEP_NOTHING.  The dictionary's
 * offsets are as wide as opts->offsets64 says.  counts and *n_lines as gx_text_group_lines delivers them.  Like every gx_text_* call it
 * returns with all its work on opts->stream done. */
int gx_text_lookup_lines(gx_handle* h, const uint8_t* text, uint64_t size, const gx_group_part* parts, uint32_t n_parts,
                         const gx_where_term* terms, uint32_t n_terms, const void* entry_units, const void* entry_offsets,
                         uint64_t n_entries, uint32_t keep, uint32_t flags, const gx_lookup_out* out, uint8_t* kept, uint64_t kept_cap,
                         void* kept_offsets, uint32_t* kept_index, gx_lookup_totals* totals, uint64_t* counts, uint64_t* n_lines,
                         const gx_batch_opts* opts);

/* The whole-file form, next to gx_text_to_jsonl: one homogeneous JSON Lines stream per extraction.  The output is what
 * gx_text_to_jsonl writes with its lines regrouped stably by extraction: extraction 0's objects first, in the order of their lines,
 * then extraction 1's, and so on.  group_out (host, optional, uint64_t[K + 1]): extraction k's objects are
 * out[group_out[k] .. group_out[k + 1]), group_out[K] == *out_size.  counts (optional, uint64_t[2K + 2], host) receives the
 * histogram over the outcome index as gx_text_select gives it, *n_lines (optional) the number of lines; out == NULL only asks for the
 * sizes; GX_E_LIMIT when out_cap is too small.  Options and limits are gx_text_to_jsonl's: device_pointers (text -- 16-byte aligned
 * -- and out on the device), stream, utf8_passthrough, utf8 (1); text of 4 GiB and more must be split by the caller. */
int gx_text_to_jsonl_by_extraction(gx_handle* h, const uint8_t* text, uint64_t size, const char* id_as, uint8_t* out, uint64_t out_cap,
                                   uint64_t* out_size, uint64_t* group_out, uint64_t* counts, uint64_t* n_lines, const gx_batch_opts* opts);

/* Compact result rows for transport between GPUs (the gather of SURVEY.md section 8(e)): per line one int16 match id
 * followed by `slots` (= 2 * gx_max_groups) uint16 offsets, 0xFFFF = unset: 2 + 2*slots bytes instead of 4 + 4*slots.
 * Device buffers only.  *n_overflow (host) receives the number of offsets above 65534, which do not fit (they are
 * stored saturated): when it is not 0 the caller sends that batch in the wide format.  gx_unpack_results is the
 * inverse.  Both run on the stream in opts (NULL = the null stream); pack synchronises it to read the counter. */
int gx_pack_results(const int32_t* match_id, const int32_t* caps, uint64_t n, int32_t slots, uint16_t* packed,
                    uint64_t* n_overflow, const gx_batch_opts* opts);
int gx_unpack_results(const uint16_t* packed, uint64_t n, int32_t slots, int32_t* match_id, int32_t* caps,
                      const gx_batch_opts* opts);
/* The same from the u8 rows of gx_batch_opts.compact_results = 2 (int8 id, uint8 offsets, 0xFF = unset). */
int gx_unpack_results8(const uint8_t* rows, uint64_t n, int32_t slots, int32_t* match_id, int32_t* caps,
                       const gx_batch_opts* opts);

/* Names for a handle built from regex strings (the caller did DefinitionReader's work itself and holds the
 * CookedExtraction data, core/model/CookedExtraction.java:18-66): extraction name, extractor names in group
 * order (n_names == gx_num_groups(h, k)), and the `append` object as JSON text (NULL = none). */
int gx_set_extraction_meta(gx_handle* h, int32_t k, const char* name, const char* const* extractor_names, int32_t n_names,
                           const char* append_json);

/* How a captured value is read as a number.  The reference's caller does not only Long.parseLong what a line captured
 * (README.md:26,63-79): its next line is as often Instant.parse(r.asMap().get("ts")).toEpochMilli() or
 * new BigDecimal(r.asMap().get("request_time")).  A FORMAT {kind, scale} is a property of group g of extraction k, kept on the
 * handle like the names of gx_set_extraction_meta.  Wherever a call parses that group as a number -- the GX_WHERE_INT_* terms of
 * gx_select_lines_where, a measure of gx_capture_stats, the value group of gx_group_lines / gx_group_quantiles / gx_top_groups /
 * gx_top_lines / gx_capture_quantiles, both groups of a gx_bucket_lines part (origin and width are in the number group's unit), and
 * their gx_text_* forms -- it parses it under the group's format, and a term's `number`,
 * a measure's `edges` and every min / max / sum / quantile / ranked value are in the format's unit.  Nothing else sees the format:
 * text terms, keys, the extraction itself and JSON Lines read the value as text.  The rule: gorp_amd/csrc/gx_number.hpp.
 *   GX_NUMBER_LONG     scale 0: Long.parseLong on ASCII.  The default of every group.
 *   GX_NUMBER_DECIMAL  scale 0 .. 18: [+-]? ( digits+ ( '.' digits* )? | '.' digits+ ), the value times 10^scale with further
 *                      fraction digits dropped toward zero: new BigDecimal(t).setScale(scale, RoundingMode.DOWN).unscaledValue()
 *                      .longValueExact().  No exponent, no grouping.  "-0.0004" at scale 3 is 0; "12.7" at scale 0 is 12.
 *   GX_NUMBER_ISO8601  scale 0, 3, 6 or 9: YYYY-MM-DD, 'T' / 't' / one space, hh:mm:ss, an optional '.' or ',' and 1 .. 9 digits,
 *                      an optional zone: 'Z', 'z', +hh:mm, +hhmm, +hh (either sign, at most 18:00); none is UTC.  The value is the
 *                      instant in 10^-scale seconds since the epoch, further digits dropped (toEpochMilli's floor): scale 3 of
 *                      "1969-12-31T23:59:59.999Z" is -1.  Years 0001 .. 9999; year 0000, ":60", "24:00:00", date-only, week and
 *                      ordinal dates are no numbers, and at scale 9 neither is an instant outside int64 nanoseconds.
 *   GX_NUMBER_CLF      scale 0, 3, 6 or 9: the access-log stamp "dd/Mon/yyyy:HH:mm:ss +hhmm", exactly
 *                      (DateTimeFormatter.ofPattern("dd/MMM/yyyy:HH:mm:ss Z", Locale.ENGLISH)).
 * Whatever fits no grammar or lies outside int64 is "not a number", as today.  RFC 3164 stamps carry no year: out of scope.
 * The setters need no device (a host-only handle takes them) and must not run concurrently with a call on the handle.  The format
 * is not part of the blob: gx_blob_copy gives the same bytes before and after, and a handle from a blob -- each handle of
 * gx_create_on_devices too -- starts with LONG everywhere.  GX_E_ARG: h / k / g out of range, an unknown kind, a scale the kind does
 * not take.  f == NULL sets the group back to LONG.
 * gx_parse_number is the rule on the host: units[0, n_units) (bytes, or 16-bit units with utf16 != 0) under *f (NULL: LONG);
 * *is_number = 0 / 1, and *value when it is 1.  It is how a caller turns "2026-01-03T00:00:00Z" into a term's `number`. */
enum { GX_NUMBER_LONG = 0, GX_NUMBER_DECIMAL, GX_NUMBER_ISO8601, GX_NUMBER_CLF };
typedef struct gx_number_format { uint32_t kind, scale; } gx_number_format;
int gx_set_number_format(gx_handle* h, int32_t k, int32_t g, const gx_number_format* f);
int gx_get_number_format(const gx_handle* h, int32_t k, int32_t g, gx_number_format* out);
int gx_parse_number(const gx_number_format* f, const void* units, uint32_t n_units, uint32_t utf16, int64_t* value, int32_t* is_number);

/* Replaces one Gorp.extract(String) call (core/Gorp.java:145-147): s is the
 * String's UTF-16 code units.  Runs on the GPU like the batch path.
 * caps has 2*gx_max_groups(h) slots. */
int gx_extract_one_utf16(gx_handle* h, const uint16_t* s, int32_t len, int32_t* match_id, int32_t* caps);

/* PolyMatcher.match over a batch with the full answer: states[i] = the product-DFA state line i ends in (-1: the dead
 * state, the reference's early return, core/autom/PolyMatcher.java:128-130); gx_state_accepts(h, state, ...) is
 * Automata.accept(state) (core/autom/Automata.java:137-139): all extraction indexes accepting there, ascending
 * (returns the count, <= cap written; 0 for -1).  first_match[i] = their first element or -1, as with
 * gx_extract_batch + match_only.  Runs on the tile kernel where the automaton's dense rows are the tables (in LDS, or in global
 * memory: a row is a state), else on the per-line kernel (the record and hop tables keep only the first match). */
int gx_match_batch(gx_handle* h, const uint8_t* bytes, const void* offsets, uint64_t n, int32_t* first_match,
                   int32_t* states, const gx_batch_opts* opts);
int gx_state_accepts(const gx_handle* h, int32_t state, int32_t* indexes, int32_t cap);

/* Replaces CookedExtraction.match(String) (core/model/CookedExtraction.java:61; JDKRegexpCookedExtraction.match,
 * core/jdkre/JDKRegexpCookedExtraction.java:36-39) -- the product of the reference's plugin seam, ExtractionCooker.cook
 * (core/ExtractionCooker.java:22): extraction k's capture regexp alone against one String, no matcher stage.
 * *matched = 1 and caps filled (2*gx_max_groups(h) slots) when the regexp matches the whole line, else 0 (the reference
 * returns null). */
int gx_capture_one_utf16(gx_handle* h, int32_t k, const uint16_t* s, int32_t len, int32_t* matched, int32_t* caps);

/* Replaces PolyMatcher.match(CharSequence) -> int[] (core/autom/PolyMatcher.java:123-133):
 * all matching extraction indexes, ascending.  Returns the count (<= cap written), or <0 on error. */
int gx_match_one_utf16(gx_handle* h, const uint16_t* s, int32_t len, int32_t* indexes, int32_t cap);

/* Definition-time string rewriting that defines the two regex dialects
 * (RegexHelper.quoteLiteralAsRegexp core/util/RegexHelper.java:20-70,
 *  massageRegexpForAutomaton :79-182, massageRegexpForJDK :210-237), used by
 * Gorp._buildExtractor (core/Gorp.java:94-129) to produce the inputs of
 * gx_create_from_patterns.  UTF-8 in, NUL-terminated UTF-8 out; *out_len
 * receives the length without the NUL.  GX_E_ARG with *out_len set when cap
 * is too small; GX_E_REGEX_SYNTAX for the IllegalArgumentException cases. */
int gx_quote_literal_as_regexp(const char* text, char* out, size_t cap, size_t* out_len);
int gx_massage_regexp_for_automaton(const char* pattern, char* out, size_t cap, size_t* out_len);
int gx_massage_regexp_for_jdk(const char* pattern, char* out, size_t cap, size_t* out_len);

/* Native front-end for the definition language (.grp text): replaces
 * DefinitionReader.reader(String).read() (core/DefinitionReader.java:58-84) -- tokenising
 * (:126-181,189-640), pattern / template / extraction resolution (core/model/CookedDefinitions.java:57-453)
 * and Gorp.construct (core/Gorp.java:50-92).  GX_E_DEFINITION carries the reference's
 * DefinitionParseException text, "([source (row,col)]): message".
 * gx_definition_to_json returns what the reference keeps in Java objects: stage "flattened" = per
 * extraction its name, flattened pieces, extractor names (capture-group order), `append` object and the two
 * regex strings; stages "uncooked" / "cooked" expose the intermediate piece lists that the reference's own
 * parser tests assert on.  NUL-terminated UTF-8 out; *out_len = length without the NUL (GX_E_ARG with
 * *out_len set when cap is too small). */
int gx_create_from_definition(const char* definition_text, const char* source_ref, uint32_t flags, gx_handle** out);
int gx_definition_to_json(const char* definition_text, const char* source_ref, const char* stage,
                          char* out, size_t cap, size_t* out_len);
/* Metadata of a handle built by gx_create_from_definition or completed with gx_set_extraction_meta (NULL otherwise /
 * out of range); strings live as long as the handle (or until the next gx_set_extraction_meta).  CookedExtraction.getName() (core/model/CookedExtraction.java:36), the extractor names in
 * capture-group order (FlattenedExtraction.getExtractorNames()), and getExtra() as JSON object text. */
const char* gx_extraction_name(const gx_handle* h, int32_t k);
const char* gx_extractor_name(const gx_handle* h, int32_t k, int32_t g);
const char* gx_extraction_append_json(const gx_handle* h, int32_t k);
/* getExtra() entry by entry, in order: the key (decoded, UTF-8) and the value as JSON text (a string value keeps
 * its quotes and escapes); count = 0 when the extraction appends nothing. */
int32_t gx_extraction_append_count(const gx_handle* h, int32_t k);
const char* gx_extraction_append_key(const gx_handle* h, int32_t k, int32_t j);
const char* gx_extraction_append_value_json(const gx_handle* h, int32_t k, int32_t j);

/* Thread-local message for the last failing call on this thread. */
const char* gx_last_error(void);

/* Devices.  A handle lives on the device that is current for the calling thread when it is created (HIP's per-thread
 * current device; device 0 unless gx_set_device was called on that thread) and every call on the handle runs there,
 * whichever thread makes it.  One process drives several GPUs with one handle per device -- built from the same
 * definition, or from one blob (gx_create_from_blob) -- and either its own threads, each calling gx_extract_batch on
 * its handle (Gorp "may be used concurrently", core/Gorp.java:22), or gx_extract_batch_multi below. */
int gx_device_count(void);
/* gx_split_lines / gx_split_lines_max keep one workspace per device between calls (an eighth of the largest text they have seen
 * there, a quarter with line flags); this gives a device's back.  Calls on different devices do not wait for each other. */
int gx_release_scratch(int device);
int gx_set_device(int device);
int gx_handle_device(const gx_handle* h);   /* -1 for a host-only handle */

/* One CSR batch in HOST memory over several devices: the lines are cut into n_handles contiguous shards of about
 * equal bytes (lines are independent: no exchange between the shards), shard k runs on handles[k]'s device through that
 * handle's host pipeline, all shards concurrently, and the results land in the caller's arrays in line order.  The
 * handles must come from the same definition.  opts as for gx_extract_batch (host pointers only; stream is ignored). */
int gx_extract_batch_multi(gx_handle* const* handles, int32_t n_handles, const uint8_t* bytes, const void* offsets, uint64_t n,
                           int32_t* match_id, int32_t* caps, const gx_batch_opts* opts);

/* The same for batches that are RESIDENT on the devices (the one-process-many-GPUs layout without the bus in the way): shard k is a
 * CSR batch in the memory of shards[k].handle's device -- bytes / offsets / n / match_id / caps as for gx_extract_batch with
 * device_pointers, `overflow` a device uint64_t on that device (or NULL), `stream` a hipStream_t of that device (NULL: a stream the
 * handle keeps for this purpose).  One call enqueues every shard on its device from the calling thread, then -- unless
 * opts->no_sync -- waits for all of them; the shards run concurrently.  No exchange between the shards: lines are independent.
 * opts as for gx_extract_batch (device_pointers is implied; stream and overflow are per shard, those of opts are ignored).  A shard
 * that fails does not stop the others; the first failure is returned. */
typedef struct gx_device_shard {
    gx_handle* handle;
    const uint8_t* bytes;
    const void* offsets;
    uint64_t n;
    int32_t* match_id;
    int32_t* caps;
    void* overflow;
    void* stream;
} gx_device_shard;
int gx_extract_batch_multi_device(const gx_device_shard* shards, int32_t n_shards, const gx_batch_opts* opts);

/* One process, all GPUs of a node (the reference's caller is ONE JVM, "fully thread-safe and may be used concurrently",
 * core/Gorp.java:22; BASELINE north_star: "broadcast of the DFA tables and a final gather over xGMI").  Ranks of a multi-process
 * job exchange the blob and the rows with RCCL (gorp_amd/dist.py); this is the same for the caller that owns every device itself.
 *
 * gx_create_on_devices: one handle per device from ONE blob (gx_blob_copy of a handle compiled once).  handles[0] is built from
 * the blob on devices[0]; the others take their device images -- the class maps, the LDS table images, the dense rows and hop
 * records in global memory: 9 KB for the README definition, 18 MB for 512 extractions -- from devices[0]'s copy, device to device
 * (hipMemcpyPeer: over xGMI between peers; gx_stat(h, 30) = bytes that came this way), their host-side tables built in threads of
 * their own.  All or nothing: on failure every handle that was created is destroyed and handles[] is NULL.
 *
 * gx_gather_rows: the result rows of a sharded batch (gx_extract_batch_multi_device with compact_results 1 or 2; any fixed row
 * size works: dense caps rows are 8 G bytes) onto ONE device, in shard order: dst_rows[sum of n over the shards before k ...].
 * Each shard's copy is enqueued on a copy stream of the SHARD's device behind the shard's kernel (an event on `stream`: the
 * stream that kernel was enqueued on; NULL = the stream gx_extract_batch_multi_device uses when the shard brings none), as one
 * hipMemcpyPeerAsync -- seven peers push into the root over seven links at once, nothing funnels through the host.  no_sync != 0:
 * returns when everything is enqueued; gx_gather_wait(handles) waits for those copies.  The next batch's kernels may be enqueued
 * (on the kernel streams) before the gather of this one is waited for -- a two-deep pipeline with two row buffers per shard: wait
 * for gather k before batch k + 2 writes the rows gather k reads ("One process, eight GPUs"). */
typedef struct gx_rows_shard {
    gx_handle* handle;      /* names the shard's device */
    const void* rows;       /* on that device: n rows of row_bytes bytes */
    uint64_t n;
    void* stream;           /* hipStream_t the shard's kernel was enqueued on (NULL: the handle's own multi-device stream) */
} gx_rows_shard;
int gx_create_on_devices(const void* blob, size_t size, const int32_t* devices, int32_t n_devices, uint32_t flags, gx_handle** handles);
int gx_gather_rows(const gx_rows_shard* shards, int32_t n_shards, uint32_t row_bytes, int32_t dst_device, void* dst_rows, int32_t no_sync);
int gx_gather_wait(gx_handle* const* handles, int32_t n_handles);

/* Host buffers that are handed to gx_extract_batch again and again (a JNI caller's direct ByteBuffers) can be pinned
 * once: copies from and to pinned memory run at the bus' rate without a staging copy by the CPU (hipHostRegister /
 * hipHostUnregister). */
int gx_host_register(void* p, size_t bytes);
int gx_host_unregister(void* p);

#ifdef __cplusplus
}
#endif
#endif /* GORP_HIP_H */
