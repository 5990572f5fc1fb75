/*
 * frender_amd.h — C ABI of libfrender_hip.so, the MI355X (gfx950) implementation of
 * frender's `scan` hot path: per-read header scan + barcode tally, Hamming
 * classification of the unique index combos, and the -rc per-sample call.
 *
 * The reference (njspix/frender, frender.py) has no FFI; its seam is three Python
 * calls inside frender_scan (frender.py:606, :610/:628, :614).  The entry points
 * below replace exactly those calls (each cites the reference function it
 * replaces); the host CLI (frender_amd/scan.py) keeps the reference's flags and
 * CSV formats and binds this header through ctypes (frender_amd/_lib.py).
 *
 * Conventions: every int-returning call returns FR_OK (0) or an FR_ERR_* code and
 * leaves a message in fr_last_error(ctx).  All pointers are plain host pointers
 * unless the name says _device.  Caller owns inputs; the library owns device
 * memory and the arrays it hands back until the next call that rebuilds them.
 * One context = one GPU = one host thread (not re-entrant).
 */
#ifndef FRENDER_AMD_H
#define FRENDER_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FR_OK 0
#define FR_ERR_INVALID 1   /* bad argument / call order */
#define FR_ERR_HIP 2       /* HIP runtime error */
#define FR_ERR_CAPACITY 3  /* a device table or pool is full */
#define FR_ERR_DEVICE 4    /* a kernel reported an internal failure (look-back spin bound) */
#define FR_ERR_IO 6        /* a .gz input could not be inflated (fr_gz_feed; message in fr_gz_error) */

/* scan-time data errors: reported in fr_file_stats.error, mirroring the reference's crash */
#define FR_SCAN_OK 0
#define FR_SCAN_NO_SPACE 1 /* header line without ' ': IndexError at frender.py:169 */
#define FR_SCAN_UTF8 2     /* invalid UTF-8: UnicodeDecodeError from gzip.open(...,"rt") at :159 */

/* classification classes (read_type, frender.py:266-284) */
#define FR_UNDETERMINED 0
#define FR_INDEX_HOP 1
#define FR_DEMUXABLE 2
#define FR_AMBIGUOUS 3

typedef struct fr_ctx fr_ctx;

/* Lines end at "\r\n", '\r' or '\n' (a '\r' that is the data's last byte ends its line: nothing follows it);
 * a last line without a terminator counts.  A header without ' ' is a record like any other but tallies no
 * code, and the tally goes on past it: the other headers of the file are counted as usual (the host raises the
 * reference's error from `error`).  With -s nothing past the last sampled header is tallied or is an error, and
 * `lines` and `utf8_bad` are those of the bytes the library scanned, which reach at least to the last sampled
 * header and at most to the file's end (fr_feed_device scans the whole file; fr_feed stops at a line end of its
 * own choosing once the sample is complete): 4 * records - 3 <= lines <= the file's lines. */
typedef struct fr_file_stats {
    uint64_t records;        /* header lines counted (after -s), = `actual_reads` (frender.py:160-166) */
    uint64_t lines;          /* lines in the file (universal newlines) */
    uint64_t new_keys;       /* distinct codes in this file, exotic ones included (`new_barcodes`, :175) */
    uint64_t exotic;         /* records whose code is outside both key forms (see fr_get_exotic_table) */
    int32_t error;           /* FR_SCAN_* (FR_SCAN_NO_SPACE wins when both were seen) */
    int32_t utf8_bad;        /* 1: an invalid UTF-8 sequence lies in the bytes scanned (with -s possibly past the
                              * sample: the host decides whether the reference's reader would decode it) */
    uint64_t error_offset;   /* file byte offset of the first offending header (FR_SCAN_NO_SPACE) */
} fr_file_stats;

typedef struct fr_timing {
    uint64_t scan_launches;  /* tally kernel launches since fr_reset */
    uint64_t scan_bytes;     /* decoded bytes those launches scanned */
    double scan_ms;          /* summed HIP-event duration of those launches */
    double last_scan_ms;     /* duration of the most recent launch */
    double classify_ms;      /* last classify pass */
    double finalize_ms;      /* last compaction + ordering */
    double log_ms;           /* summed duration of the launch-log aggregations after those launches */
} fr_timing;

/* ---- lifecycle ------------------------------------------------------------------ */
/* chunk_bytes: bytes per tally launch of a device feed, at most 16 GiB - 1 MiB (device feeds are cut
 * into equal ranges of at most this size, and of at most 4 GiB - 1 MiB while their commits may go to
 * the launch log; host feeds use a pinned ring of min(chunk_bytes, 1 GiB) slots).
 * table_slots: initial HBM hash-table slots (grown between launches).  Nothing in the environment
 * changes a context's geometry: fr_create uses the library's defaults, fr_create_tuned the caller's
 * fr_tuning (tests, A/B runs). */
fr_ctx* fr_create(int device, uint64_t chunk_bytes, uint64_t table_slots);
/* The tally's launch geometry and thresholds.  Results never depend on them (every setting gives the
 * same table); only the speed does.  Fill with fr_tuning_defaults, change fields, pass to
 * fr_create_tuned.  `size` = sizeof(fr_tuning) of the caller (fields past it keep their defaults). */
typedef struct fr_tuning {
    uint32_t size;
    int32_t grid;               /* tally workgroups; 0 = CUs x the kernel's occupancy */
    uint32_t flush_at;          /* LDS-table keys per chunk before new codes go to the cold list */
    uint32_t cold_cap;          /* cold-list entries per workgroup (>= 1024) */
    int32_t log;                /* 1: heavy commits may go to the launch log; 0: every commit inserts directly */
    uint32_t log_min;           /* pairs from which a commit logs (0: every commit) */
    uint32_t log_hot;           /* a logged commit's LDS entries of >= log_hot records insert directly (>= 1) */
    uint32_t chunk_tiles;       /* 4-KiB wave-tiles per full chunk (>= 2) */
    uint32_t chunk_tiles_heavy; /* the same once commits log (>= 2) */
    int32_t ramp;               /* 1: ramped chunk sizes; 0: one uniform chunk per workgroup */
    uint32_t ramp_up_s;         /* the ramps' smallest chunks (tiles, >= 1) */
    uint32_t ramp_down_s;
    uint32_t ramp_down_pct;     /* ramp-down chunks, % of the grid (1..100), normal / heavy geometry */
    uint32_t ramp_down_pct_h;
    int32_t spec_commit;        /* 1: device feeds commit speculative chunks at once (checked at the launch end) */
    int32_t nbr;                /* 1: classify through the sheet's neighbourhood maps; 0: row scan only */
    uint64_t ovf_cap;           /* overflow-list entries (new codes a launch adds past the table's probe bound;
                                 * 0 = 4 Mi; a device feed that overflows it is replayed in smaller ranges) */
} fr_tuning;
void fr_tuning_defaults(fr_tuning* t);
fr_ctx* fr_create_tuned(int device, uint64_t chunk_bytes, uint64_t table_slots, const fr_tuning* t);
void fr_destroy(fr_ctx* ctx);
const char* fr_last_error(const fr_ctx* ctx);
int fr_get_timing(fr_ctx* ctx, fr_timing* out);
/* on != 0 (the default): HIP timing events around every tally launch, its launch-log aggregation,
 * fr_finalize and fr_classify (fr_get_timing's figures).  on = 0: none are recorded (each event
 * record is a bubble of a few microseconds on the stream); fr_get_timing then reports zeros for the
 * work done while off.  Results do not depend on it. */
int fr_set_timing(fr_ctx* ctx, int on);
int fr_sync(fr_ctx* ctx);
/* diagnostics: {look-back max polls, total polls, keys, overflow, presence, exotic, grid, slots,
 * 8 phase stamps, speculation replays, exotic-only replays, next full-chunk size, heavy launches,
 * big-feed rollbacks, the last device feed's fullest launch-log fold, its fold overflows, its range bytes,
 * memsets and copies queued on the context's stream since the last fr_reset (each a blit dispatch of its own:
 * a steady one-file fr_feed_device step queues none), 1 when the classify neighbourhood maps were on for the
 * context's last fr_classify / fr_classify2 / fr_dmx_set_sheet* (0: every code took the row scan); a call that
 * is refused for its arguments before it looks at the maps (no sheet, rc_mode on a single-index sheet) leaves
 * the entry as the call before it set it}.  New entries are added at the end. */
int fr_get_diag(fr_ctx* ctx, uint64_t* out, int n);

/* ---- sample sheet (the idx1/idx2/id lists of get_indexes, frender.py:90-116) -------
 * idx*_packed: each entry case-folded (str.lower(), :226) and packed 3 bits/char,
 * char i at bits [3i,3i+3): a=1 c=2 g=3 t=4 n=5, any other char=7; entries longer
 * than 21 chars pack as 0 (they can only fail the length assert).  idx2rc_packed is
 * the same for reverse_complement(idx2) (:210-211).  idx*_len are the case-folded
 * lengths.  name_id[i] = index of row i's id among the distinct ids in
 * first-appearance order (call_rc_mode_per_id's dict, :367).  The code-point
 * arrays (stride `cp_stride`, may be NULL) feed the generic classifier used for
 * codes outside the fast alphabet. */
int fr_set_sheet(fr_ctx* ctx, int S,
                 const uint64_t* idx1_packed, const int32_t* idx1_len,
                 const uint64_t* idx2_packed, const int32_t* idx2_len,
                 const uint64_t* idx2rc_packed, const int32_t* name_id, int n_names,
                 const uint32_t* idx1_cp, const uint32_t* idx2_cp, const uint32_t* idx2rc_cp,
                 int cp_stride);
/* Index mode of the context (FR_INDEX_DUAL when it is created; fr_reset keeps it).  It takes effect at the next
 * fr_set_sheet.  FR_INDEX_SINGLE, for single-indexed libraries (one barcode per read, no index 2 in the
 * sheet): fr_set_sheet reads no idx2 argument (they may be NULL) and uploads every idx2 as the empty
 * string, and on such a sheet fr_classify, fr_dmx_set_sheet's records and fr_classify_cp's callers take a code
 * as its idx1 alone: code.split("+")[0], every character when it has no '+', against the empty idx2.  So a
 * code is classified as the reference classifies idx1 + "+" against a sheet whose idx2 are all "": with M the
 * rows whose idx1 is within num_subs mismatches, undetermined (|M| = 0), demuxable (1) or ambiguous (>= 2,
 * m1 = the first of them); never an index hop, m2 = 0 (the empty entry) whenever m1 >= 0.  Only idx1's length
 * is asserted (error 1); errors 2 and 3 and FR_DMX_LEN2 / FR_DMX_NOPLUS do not occur.  rc_mode is refused. */
#define FR_INDEX_DUAL 0
#define FR_INDEX_SINGLE 1
int fr_set_index_mode(fr_ctx* ctx, int mode);

/* ---- tally: replaces tally_barcodes (frender.py:183-207) / scan_file (:154-181) ----
 * Files are fed in parse_files order (:604); fr_reset starts a new scan. */
int fr_reset(fr_ctx* ctx);
int fr_begin_file(fr_ctx* ctx, int64_t max_records /* -s, <=0: no limit */);
/* fr_begin_file at a global position, for scans sharded over contexts / GPUs (SURVEY §8(e);
 * replaces the per-file work unit of the reference's Pool, frender.py:189-193): file_index is the
 * file's index in the whole scan's parse_files order and byte_base the file offset of the first
 * byte this context will be fed (a record-aligned shard of the file; 0 for a whole file).  The
 * ordinals ((file_index+1) << 44 | byte_base + offset), the presence pairs' file index and
 * therefore the merged first-occurrence order are the single-context ones.  file_index must
 * increase within a scan (fr_begin_file takes the next index). */
int fr_begin_file_at(fr_ctx* ctx, int64_t file_index, uint64_t byte_base, int64_t max_records);
/* Decoded (gunzipped) bytes of the current file, any split; the library cuts at
 * line ends, carries the remainder, copies through a pinned ring to HBM and
 * launches.  Returns FR_OK, or 5 (FR_SAMPLE_DONE) once -s records were seen. */
#define FR_SAMPLE_DONE 5
int fr_feed(fr_ctx* ctx, const uint8_t* data, uint64_t len);
/* ---- native inflate: replaces gzip.open(file, "rt") (frender.py:159) as
 * the source of the decoded bytes.  fr_gz_open starts `threads` host threads that inflate the
 * listed .gz files (zlib; multi-member, NUL padding between members as Python's gzip) up to
 * `threads` files ahead of the consumer, in list order, into 16 MiB blocks.  fr_gz_feed hands
 * file i's blocks to fr_feed (call it between fr_begin_file[_at] and fr_end_file; files in list
 * order) and returns FR_OK, FR_SAMPLE_DONE, or FR_ERR_IO when the stream is not valid gzip (the
 * caller re-reads the file with Python's gzip to raise the reference's exception). */
typedef struct fr_gz fr_gz;
fr_gz* fr_gz_open(const char* const* paths, int n_files, int threads);
/* the same with at most files_ahead files inflating at once: the other threads help split the big
 * single-member files among them (the demux reads a file pair at a time) */
fr_gz* fr_gz_open_ahead(const char* const* paths, int n_files, int threads, int files_ahead);
int fr_gz_feed(fr_gz* g, int i, fr_ctx* ctx);
/* The consumer-side alternative to fr_gz_feed (demux reads R1 and R2 in lockstep): the next decoded
 * block of file i.  *data / *len stay valid until the next fr_gz_next or fr_gz_close on the pool;
 * *len == 0 at the file's end.  FR_ERR_IO: not a valid gzip stream (fr_gz_error).  Replaces the
 * reference's gzip.open(read_file, "rt") iteration in frender_demux (frender.py:776-777). */
int fr_gz_next(fr_gz* g, int i, const uint8_t** data, uint64_t* len);
/* Record shards of one file (multi-GPU scans of fewer files than GPUs; SURVEY §8(e) "host cuts
 * record-aligned chunks and deals them to GPUs"): part `part` of `nparts` of file i's decoded
 * stream is [b_part, b_part+1), b_0 = 0, b_nparts = the end, and for 0 < j < nparts b_j = the first
 * record start (a line start whose index from the file start is 0 mod 4, universal newlines as
 * frender.py:159 reads them) at or after j * hint / nparts.  The function inflates the file from its
 * start, counts line ends on the host, calls fr_begin_file_at(ctx, file_index, b_part, 0) once the
 * part's start is known, feeds only the part's bytes, stops inflating at its end and stores b_part
 * in *byte_base; the caller then calls fr_end_file.  Every rank that passes the same `hint` cuts the
 * same way.  Not with -s (a sample is the head of each whole file). */
int fr_gz_feed_part(fr_gz* g, int i, fr_ctx* ctx, int64_t file_index, int part, int nparts, uint64_t hint,
                    uint64_t* byte_base);
/* The cuts fr_gz_feed_part makes: bounds[0..nparts] (b_0 = 0, b_nparts = the decoded size).  Host
 * only (no GPU context): FR_OK, or FR_ERR_IO when the file is not valid gzip. */
int fr_gz_part_bounds(const char* path, int nparts, uint64_t hint, uint64_t* bounds);
/* BGZF record parts without a prefix inflate (multi-GPU scans of fewer files than GPUs): a BGZF
 * file's members give every member's decoded offset from the headers alone, so part `part` of
 * `nparts` is decoded on its own.  Its member range is [M_part, M_part+1), M_j = the decoded offset of
 * the first member starting at or after j * total / nparts (M_0 = 0, M_nparts = the decoded size).
 * fr_gz_part_open decodes that range (threads: this thread plus helpers; libdeflate when present,
 * else zlib) and returns the line terminators whose terminating byte lies in it (universal newlines,
 * frender.py:159); *is_bgzf = 0 (and no handle) when the file is not BGZF: cut it with
 * fr_gz_feed_part instead.  FR_ERR_IO: a member does not decode (the host replays the file through
 * Python's gzip for the reference's exception).  With lines_before = the terminators before M_part
 * (the other parts' counts, exchanged by the caller), the part's records are [b_part, b_part+1), b_j =
 * the first record start at or after M_j: fr_gz_part_data hands them out (host bytes, valid until
 * fr_gz_part_close), fr_gz_part_feed calls fr_begin_file_at(ctx, file_index, b_part, 0) and fr_feed
 * with them (the caller then calls fr_end_file).  *inflated: decoded bytes produced for the part so far
 * (the part plus at most the members around its ends). */
typedef struct fr_gz_part fr_gz_part;
int fr_gz_part_open(const char* path, int part, int nparts, int threads, fr_gz_part** out, int* is_bgzf,
                    uint64_t* lines, uint64_t* inflated);
int fr_gz_part_data(fr_gz_part* p, uint64_t lines_before, const uint8_t** data, uint64_t* len, uint64_t* byte_base,
                    uint64_t* inflated);
int fr_gz_part_feed(fr_gz_part* p, fr_ctx* ctx, int64_t file_index, uint64_t lines_before, uint64_t* byte_base);
const char* fr_gz_part_error(const fr_gz_part* p);
void fr_gz_part_close(fr_gz_part* p);
/* The decoded size of a .gz file as far as its trailers tell (0 when unreadable): exact for BGZF (the
 * members' ISIZE fields) and for a single-member file of up to 4 GiB decoded; otherwise the last
 * member's ISIZE lifted toward 4x the compressed size.  A deterministic fr_gz_feed_part hint. */
uint64_t fr_gz_size_hint(const char* path);

/* ---- scan CSV (row a9; replaces report_analysis' csv.DictWriter, frender.py:482-501) ------------
 * Writes header, then one excel-dialect row per unique code: parts[0], parts[1] of code.split("+"),
 * matched_idx1, matched_idx2, read_type, sample_name, reads[, demux_ok].  keys[j] is row j's packed
 * key (fr_get_unique form, fast or wide); rows listed in exo_rows (increasing) take their first two
 * fields from exo_text[exo_off[e], exo_off[e+1]) instead ("p0,p1", already CSV-quoted).  dict holds
 * the CSV-quoted strings the other fields index: dict_n[0] idx1 entries (m1), dict_n[1] idx2
 * entries (m2), dict_n[2] sample names (row), dict_n[3] class names (cls); entry i is
 * dict[dict_off[i], dict_off[i+1]).  Negative m1/m2/row write an empty field; demux_ok NULL omits the
 * column.  FR_ERR_INVALID (nothing written) when a keyed code has no '+' or an index is out of
 * range; FR_ERR_IO when the file cannot be written. */
int fr_write_scan_csv(const char* path, const char* header, uint64_t n_rows, const uint64_t* keys,
                      const uint64_t* counts, const int16_t* m1, const int16_t* m2, const uint8_t* cls,
                      const int16_t* row, const uint8_t* demux_ok, const char* dict, const uint64_t* dict_off,
                      const uint32_t* dict_n, uint64_t n_exotic, const uint64_t* exo_rows, const char* exo_text,
                      const uint64_t* exo_off);
/* The same with the scan's index mode.  FR_INDEX_DUAL: fr_write_scan_csv exactly.  FR_INDEX_SINGLE: a keyed
 * code without '+' is a row too, its idx1 field the whole code and its idx2 field empty (a code with a '+'
 * splits as above, so ACGT, ACGT+ and ACGT+TTTT are three rows). */
int fr_write_scan_csv_mode(const char* path, const char* header, uint64_t n_rows, const uint64_t* keys,
                           const uint64_t* counts, const int16_t* m1, const int16_t* m2, const uint8_t* cls,
                           const int16_t* row, const uint8_t* demux_ok, const char* dict,
                           const uint64_t* dict_off, const uint32_t* dict_n, uint64_t n_exotic,
                           const uint64_t* exo_rows, const char* exo_text, const uint64_t* exo_off,
                           int index_mode);
const char* fr_gz_error(const fr_gz* g);
void fr_gz_close(fr_gz* g);
/* Decode buffers outlive their pool: a process-wide cache keeps up to 4 GiB of them for the next scan
 * (no page faults per GB).  fr_gz_trim returns every cached buffer to the OS (long-lived processes that
 * scan once, e.g. the seam, call it after a scan). */
void fr_gz_trim(void);
/* Large single-member gzip files (the usual .fastq.gz of one lane) are not one thread's work: a member of
 * at least 16 MiB compressed is decoded by all of the pool's idle threads at once (chunks of the
 * compressed stream decoded from candidate block starts with their unknown 32 KiB windows as markers,
 * stitched and resolved in order, checked against the member's CRC-32 and ISIZE; any failure decodes the
 * file with one thread instead, whose decoders own the error behaviour).  The number of files decoded
 * that way in this process (diagnostics, tests). */
uint64_t fr_gz_parallel_members(void);

/* The whole current file is already resident in HBM (bench / device producers). */
int fr_feed_device(fr_ctx* ctx, const uint8_t* dev_data, uint64_t len);
int fr_end_file(fr_ctx* ctx, fr_file_stats* out);

/* ---- the merged unique table (barcode_counter["total"], :199-203) -----------------
 * fr_finalize compacts the device hash table and orders it by first occurrence
 * (file order, then byte offset) on the GPU.  Keys: fast keys are 3-bit packed codes over
 * {A=1,C=2,G=3,T=4,N=5,'+'=6}, char i at bits [3i,3i+3), at most 21 chars; wide keys (bit 63
 * set) hold codes whose letters are all ACGTN or all acgtn, at most one '+', each part <= 21 and
 * <= 24 letters in total: bit 62 lowercase, bits 57-61 the '+' position (letters before it; 31
 * none), bits 0-56 V = sum d_i 5^i + (5^n - 1)/4 over the n letters, d: A0 C1 G2 T3 N4. */
int fr_finalize(fr_ctx* ctx, uint64_t* n_unique, uint64_t* n_presence, uint64_t* n_exotic);
int fr_get_unique(fr_ctx* ctx, uint64_t* keys, uint64_t* counts, uint64_t* first_ordinal);
/* (unique index, file index) for every file a fast-path key occurs in (R10 demux_ok) */
int fr_get_presence(fr_ctx* ctx, uint32_t* unique_idx, uint32_t* file_idx);
/* The reads of each presence pair's code in the pair's file: the values of the reference's per-file
 * tables, barcode_counter[basename][code] (scan_file's file_barcodes, frender.py:171-177, kept by
 * tally_barcodes at :204-205).  counts[n_presence] aligns with fr_get_presence, exotic_counts with
 * fr_get_exotic_table's presence pairs; either may be NULL. */
int fr_get_presence_counts(fr_ctx* ctx, uint64_t* counts, uint64_t* exotic_counts);
/* Codes outside both key forms ("exotic": mixed case, other bytes, more than 24 letters, a part
 * longer than 21, two or more '+'), aggregated over the scan by exact byte string inside the
 * library: the device captures each such record's code bytes, the library drains them after the
 * launch that produced them (a launch that overflows the list is replayed capturing exotic codes
 * only, after the list grows) and merges them natively.  Order: first drained, not first
 * occurrence (use `first`).  fr_exotic_sizes gives the array sizes for fr_get_exotic_table:
 * counts/first per code, offsets[n+1] into the concatenated code bytes, and (code, file index)
 * presence pairs (R10). */
int fr_exotic_sizes(fr_ctx* ctx, uint64_t* n_codes, uint64_t* code_bytes, uint64_t* n_presence);
int fr_get_exotic_table(fr_ctx* ctx, uint64_t* counts, uint64_t* first, uint64_t* offsets, uint8_t* bytes,
                        uint32_t* pres_code, uint32_t* pres_file);

/* ---- classify: replaces process (:391-426) -> analyze_barcodes_with_rc (:294-351)
 *      -> analyze_barcode (:237-291) -> get_indexes_of_approx_matches (:214-234) ----
 * Runs over the finalized unique table with the current sheet and num_subs.
 * Per unique (host arrays of n_unique):  m1,m2 = first matching sheet row or -1
 * (matched_idx1/2, :261-262), cls = FR_* class, row = the demux row or -1.  With
 * rc_mode the rc_* arrays receive the rc(idx2) pass and the ambiguity override
 * (:336-349) is applied; may be NULL otherwise.  err_unique receives the first
 * unique index (in order) whose lengths fail the assert at :227 (or -1), and
 * err_which 1 = idx1, 2 = idx2, 3 = no '+' (ValueError at :306). */
int fr_classify(fr_ctx* ctx, int num_subs, int rc_mode,
                int16_t* m1, int16_t* m2, uint8_t* cls, int16_t* row,
                int16_t* rc_m2, uint8_t* rc_cls, int16_t* rc_row,
                int64_t* err_unique, int32_t* err_which);
/* The same with a mismatch limit per index: idx1 is matched against the sheet's idx1 list with num_subs1
 * (:256), idx2 against the idx2 list -- and, with rc_mode, the rc(idx2) list -- with num_subs2 (:257); the
 * class rule, the rc call, the asserts and the outputs are fr_classify's.  A negative limit matches no row of
 * its list.  fr_classify(n) is fr_classify2(n, n). */
int fr_classify2(fr_ctx* ctx, int num_subs1, int num_subs2, int rc_mode,
                 int16_t* m1, int16_t* m2, uint8_t* cls, int16_t* row,
                 int16_t* rc_m2, uint8_t* rc_cls, int16_t* rc_row,
                 int64_t* err_unique, int32_t* err_which);
/* per distinct name: reads demuxable with fwd idx2 / with rc idx2 (:367-373), from the
 * last rc_mode classify */
int fr_rc_counts(fr_ctx* ctx, uint64_t* reads_f, uint64_t* reads_rc);
/* generic classifier for codes outside the fast alphabet: queries as case-folded
 * code points (stride cp_stride), same outputs as fr_classify plus a per-query err_which */
int fr_classify_cp(fr_ctx* ctx, int n, const uint32_t* q1, const int32_t* q1len,
                   const uint32_t* q2, const int32_t* q2len, int cp_stride, int num_subs, int rc_mode,
                   int16_t* m1, int16_t* m2, uint8_t* cls, int16_t* row,
                   int16_t* rc_m2, uint8_t* rc_cls, int16_t* rc_row, int32_t* err_which);
/* the same with a limit per index, as fr_classify2; fr_classify_cp(n) is fr_classify_cp2(n, n) */
int fr_classify_cp2(fr_ctx* ctx, int n, const uint32_t* q1, const int32_t* q1len,
                    const uint32_t* q2, const int32_t* q2len, int cp_stride, int num_subs1, int num_subs2,
                    int rc_mode, int16_t* m1, int16_t* m2, uint8_t* cls, int16_t* row,
                    int16_t* rc_m2, uint8_t* rc_cls, int16_t* rc_row, int32_t* err_which);

/* ---- multi-GPU merge: export / import the compacted table ----------- */
int fr_export_unique_device(fr_ctx* ctx, void* dev_keys, void* dev_counts, void* dev_first, uint64_t cap);
/* The same rows as one int64 array [U][3] of (key, count, first), partitioned by owner rank: owner = the top 24
 * bits of key * 0x9E3779B97F4A7C15 (mod 2^64) mod world (frender_amd/dist.py owner_of), the blocks of owners
 * 0..world-1 contiguous in that order (order inside a block not fixed); dev_counts receives 2 x world int64:
 * the rows per owner, then scratch.  Synchronises the library's stream.  1 <= world <= 1024. */
int fr_export_partitioned_device(fr_ctx* ctx, int world, void* dev_rows, void* dev_counts, uint64_t cap);
/* Merge n int64 rows [n][3] (key, count, first) from device memory into the table (count = sum, first = min);
 * the row-major form of fr_merge_unique_device (the rows an all-to-all delivered). */
int fr_merge_rows_device(fr_ctx* ctx, const void* dev_rows, uint64_t n);
int fr_merge_unique_device(fr_ctx* ctx, const void* dev_keys, const void* dev_counts, const void* dev_first,
                           uint64_t n);

/* ---- device memory + SYN-v1 generator (bench and tests) --------------------------- */
void* fr_device_alloc(fr_ctx* ctx, uint64_t bytes);
int fr_device_free(fr_ctx* ctx, void* ptr);
int fr_copy_to_host(fr_ctx* ctx, void* dst, const void* dev_src, uint64_t bytes);
int fr_copy_to_device(fr_ctx* ctx, void* dev_dst, const void* src, uint64_t bytes);
/* records r0..r0+n-1 of SYN-v1 (frender_amd/synth.py) into dev_out; idx ascii S*L */
int fr_synth_device(fr_ctx* ctx, uint8_t* dev_out, uint64_t r0, uint64_t n, int R, uint64_t seed,
                    const char* idx1_ascii, const char* idx2_ascii, int S, int L1, int L2);

/* ---- demux: replaces the hot loop of frender_demux (frender.py:776-810)
 * One file pair at a time.  The caller hands over decoded text with universal newlines already
 * normalised to '\n' (the reference reads in text mode, :776).  Records are groups of 4 lines
 * (grouper, :719-723); the R2 record's code is the text after the last ':' of its first line
 * (:778).  Destinations are small non-negative ids chosen by the caller (one per writer pair). */
#define FR_DMX_MISSING (-1) /* code not in the results: SystemExit "Couldn't find barcode ..." (:807-810) */
#define FR_DMX_BADTYPE (-2) /* read type with no writers: SystemExit "Unrecognized read type ..." (:803-806) */
#define FR_DMX_EXOTIC (-3)  /* code outside the fast alphabet / > 21 chars: the host resolves it */
/* sheet mode (fr_dmx_set_sheet) only: the code's classification error, as `scan` raises it (frender.py:227-229, :306) */
#define FR_DMX_LEN1 (-4)    /* idx1's length differs from the sheet's: AssertionError */
#define FR_DMX_LEN2 (-5)    /* idx2's length differs from the sheet's: AssertionError */
#define FR_DMX_NOPLUS (-6)  /* no '+' in the code: ValueError */

typedef struct fr_dmx fr_dmx;
fr_dmx* fr_dmx_create(int device);
void fr_dmx_destroy(fr_dmx* d);
const char* fr_dmx_last_error(const fr_dmx* d);
/* results table: fast-alphabet codes (3-bit packed like fr_get_unique keys) -> destination or
 * FR_DMX_BADTYPE; codes absent from the table resolve to FR_DMX_MISSING */
int fr_dmx_set_table(fr_dmx* d, const uint64_t* keys, const int32_t* vals, uint64_t n);
/* sheet mode, instead of a results table: every R2 record's code is classified against ctx's sheet as
 * fr_classify classifies it with num_subs and no rc (frender.py:214-291), and the record goes to
 * row_dest[row] (n_rows = the sheet's rows) when it is demuxable, else to class_dest[class] (0 undetermined,
 * 1 index hop, 3 ambiguous; entry 2 is unused); these may be FR_DMX_MISSING / FR_DMX_BADTYPE.  A code with a
 * classification error gets FR_DMX_LEN1 / _LEN2 / _NOPLUS.  ctx is a context on d's device on which
 * fr_set_sheet has been called: d borrows its device sheet and its neighbourhood maps for num_subs (built
 * here when they are not current; ctx's stream is synchronised once) until the next fr_dmx_set_table /
 * fr_dmx_set_sheet / fr_dmx_destroy.  Meanwhile the caller keeps ctx alive, leaves its sheet as it is and
 * classifies on it with no other num_subs.  fr_dmx_set_table switches back to table mode. */
int fr_dmx_set_sheet(fr_dmx* d, fr_ctx* ctx, int num_subs, const int32_t* row_dest, int n_rows,
                     const int32_t class_dest[4]);
/* the same with a limit per index, as fr_classify2 classifies (the borrowed maps are those of the pair);
 * fr_dmx_set_sheet(n) is fr_dmx_set_sheet2(n, n) */
int fr_dmx_set_sheet2(fr_dmx* d, fr_ctx* ctx, int num_subs1, int num_subs2, const int32_t* row_dest, int n_rows,
                      const int32_t class_dest[4]);
/* The mates of an input: 2 (the default: a read pair, mate 1 is the code mate) or 1, a single-end file
 * (`demux --single-end`).  With 1 there is no mate 1: mate 0 is the code mate, so fr_dmx_load* / fr_dmx_bgzf_fill
 * with mate 0 do what they do with mate 1 of a pair (count and index the records, extract every record's code: the
 * table lookup, or in sheet mode the fast key, the classification and with fr_dmx_bstats_begin the bin byte), and
 * fr_dmx_exotic / _patch / _bstats_patch / _tally_window index mate 0's records.  fr_dmx_route routes
 * min(n_pairs, mate 0's records) records with one length pass, one offset scan and one copy; every bytes_r2[k] is 0
 * and nothing of mate 1's is allocated or touched.  fr_dmx_stats_window / _cycles_window launch over one mate (the
 * accumulators keep their layout, mate 1's half stays zero); fr_dmx_validate_window needs mate 0 alone and checks
 * kinds 1-4 of its records.  Every entry point that takes a mate returns FR_ERR_INVALID for mate 1.
 * n_mates outside {1, 2} is FR_ERR_INVALID; a call that changes nothing is a no-op (so fr_dmx_set_mates(2) on a new
 * context is); a call that changes the count is FR_ERR_INVALID while a mate holds a window (the last fr_dmx_load* or
 * fill of a mate left bytes: a load of zero bytes empties it) or a BGZF mate is open.  A caller that borrowed a
 * context sets it back to 2 once its last window is done, as it calls fr_dmx_validate_end. */
int fr_dmx_set_mates(fr_dmx* d, int n_mates);
/* mate 0 = R1, 1 = R2 (R2 also resolves every record's destination); returns the record count */
int fr_dmx_load(fr_dmx* d, int mate, const uint8_t* data, uint64_t len, uint64_t* n_records);
/* the same over the concatenation of n_parts host buffers (a window without a host-side join) */
int fr_dmx_load_parts(fr_dmx* d, int mate, const uint8_t* const* parts, const uint64_t* lens, int n_parts,
                      uint64_t* n_records);
/* the same over bytes already resident in HBM (16-byte aligned; used in place until the next load) */
int fr_dmx_load_device(fr_dmx* d, int mate, const uint8_t* dev_data, uint64_t len, uint64_t* n_records);
/* byte span [start, end) of the given records of a mate (host error messages, exotic codes) */
int fr_dmx_records(fr_dmx* d, int mate, const uint64_t* recs, uint64_t n, uint64_t* starts, uint64_t* ends);
/* R2 records < n_pairs whose destination is FR_DMX_EXOTIC (first cap written; *n = total) */
int fr_dmx_exotic(fr_dmx* d, uint64_t n_pairs, uint64_t* recs, uint64_t cap, uint64_t* n);
/* set the destinations of the given R2 records (the host's resolution of exotic codes) */
int fr_dmx_patch(fr_dmx* d, const uint64_t* recs, const int32_t* dest, uint64_t n);
/* route the first n_pairs record pairs: if some pair has a negative destination, *first_error is
 * the first such pair and *error_val its value (nothing routed); otherwise both mates' records
 * are gathered destination-major (record order kept within a destination) and the byte count
 * of every destination is returned per mate.  With no negative destination among them, a destination
 * >= n_dest is FR_ERR_INVALID ("fr_dmx_route: destination out of range"): nothing is routed, fr_dmx_fetch
 * has no bytes and no fr_dmx_tally_window / fr_dmx_stats_window / fr_dmx_cycles_window is pending */
int fr_dmx_route(fr_dmx* d, int n_dest, uint64_t n_pairs, int64_t* first_error, int32_t* error_val,
                 uint64_t* bytes_r1, uint64_t* bytes_r2);
/* the routed bytes of a mate (destination-major) */
int fr_dmx_fetch(fr_dmx* d, int mate, uint8_t* out, uint64_t len);
/* the demux writers' compression on the GPU (replaces the gzip.open(..., "wb") writer pairs of
 * frender.py:667-676 that frender.py:795-810 write every routed record to): the routed bytes of a mate
 * (the last fr_dmx_route) become one raw deflate stream (RFC 1951) per destination that has bytes;
 * comp_bytes[k] = its byte count (0: no bytes routed), crc32[k] = the CRC-32 of destination k's routed
 * bytes, so that a gzip member is header + stream + (crc32[k], bytes routed).  The streams stay on the
 * device, destination-major, until fr_dmx_fetch_deflated (the next fr_dmx_deflate of the mate replaces
 * them). */
int fr_dmx_deflate(fr_dmx* d, int mate, int n_dest, uint64_t* comp_bytes, uint32_t* crc32);
int fr_dmx_fetch_deflated(fr_dmx* d, int mate, uint8_t* out, uint64_t len);
/* the same bytes as BGZF (fr_defl_run_bgzf): every destination that has bytes becomes a run of complete
 * BGZF members, comp_bytes[k] = the run's byte count with its framing (0: no bytes routed).  The runs are
 * fetched with fr_dmx_fetch_deflated and appended to the destination's file as they are; the file's one
 * EOF block is the host's to write. */
int fr_dmx_deflate_bgzf(fr_dmx* d, int mate, int n_dest, uint64_t* comp_bytes);

/* ---- the demux windows' tally (`demux -b --report`; fr_dmx_tally.hip): the scan's table of every distinct
 * code, counted over the R2 record keys of the windows a one-pass demux routes, so that one pass over the inputs
 * gives the output files and the results CSV.  Sheet mode only, off until fr_dmx_tally_begin; the table persists
 * over all windows and file pairs until the next fr_dmx_tally_begin or fr_dmx_destroy.  Only fast keys are
 * counted here: a record fr_dmx_exotic reports is the host's to count, by its string.  Every call below returns
 * FR_ERR_INVALID in table mode or before fr_dmx_tally_begin, and FR_ERR_CAPACITY (never a wrong count) when a
 * table could not take an entry. */
/* Start (or clear) the tally.  initial_slots: the HBM table's first size (0: 64 Ki slots; rounded up to a power
 * of two, at least 64); before a window is counted the table has at least twice as many slots as (distinct keys
 * so far + the window's pairs), or is rebuilt larger on the device. */
int fr_dmx_tally_begin(fr_dmx* d, uint64_t initial_slots);
/* The windows that follow belong to file pair file_index (increasing within a tally, below 2^19): a record's
 * ordinal is (file_index + 1) << 44 | its index among the pair's records, which orders records as scan's
 * ordinals do (file order, then position).  Closes the previous pair: its reads per code become presence
 * entries, the per-file tables scan_file returns (frender.py:171-177) and tally_barcodes keeps (:204-205). */
int fr_dmx_tally_file(fr_dmx* d, int64_t file_index);
/* Count the n_pairs records the last fr_dmx_route routed (that call found no negative destination among them;
 * n_pairs must be its count, and a window is counted once): count += 1 and first = min(ordinal) per code, the
 * merged table of tally_barcodes (frender.py:199-203).  first_record: the index, within the file pair, of the
 * window's first record.  Records past n_pairs carry into the next window and are counted there.  Makes no
 * synchronisation of its own. */
int fr_dmx_tally_window(fr_dmx* d, uint64_t n_pairs, uint64_t first_record);
/* Closes the last pair; the sizes of fr_dmx_tally_get's arrays. */
int fr_dmx_tally_sizes(fr_dmx* d, uint64_t* n_unique, uint64_t* n_presence);
/* The table as host arrays, in no fixed order: keys (3-bit packed like fr_get_unique's fast keys), counts and
 * first ordinals per code (barcode_counter["total"], frender.py:199-203), and per (code, file pair) with reads
 * the code's index in keys, the pair's file index and its reads there (barcode_counter[basename][code],
 * :204-205; fr_get_presence and fr_get_presence_counts in one). */
int fr_dmx_tally_get(fr_dmx* d, uint64_t* keys, uint64_t* counts, uint64_t* first, uint32_t* pres_unique,
                     uint32_t* pres_file, uint64_t* pres_reads);
/* The same codes as int64 rows [n_unique][3] of (key, count, first) in device memory (cap rows), the form
 * fr_merge_rows_device takes; complete when the call returns. */
int fr_dmx_tally_rows_device(fr_dmx* d, void* dev_rows, uint64_t cap);

/* ---- the demux windows' per-output statistics (`demux --stats`; fr_dmx_stats.hip): what every destination got,
 * per mate, summed over the routed records while they are resident: table mode and sheet mode alike.  A record
 * is fr_dmx_records' byte span (up to four lines; a file's partial last group counts); split at its '\n', its
 * second piece is the sequence and its fourth the quality line (absent pieces are empty).  Per record:
 * reads += 1, bases += the sequence's length, quality_bytes += the quality line's length, q30_bases += its bytes
 * with unsigned value >= 63 ('?', Phred+33 Q30), quality_raw_sum += its unsigned byte values (no byte is
 * special; the caller subtracts 33 per quality byte).  Every call below returns FR_ERR_INVALID, with the sums
 * untouched, when the order described is not kept. */
/* Start (or clear) the statistics of a demux: n_dest destinations, all sums zero.  Off until this call. */
int fr_dmx_stats_begin(fr_dmx* d, int n_dest);
/* Add the n_pairs record pairs the last fr_dmx_route routed (it found no negative destination; n_pairs must be
 * its count; a window is added once; before the next fr_dmx_load*; that route's n_dest is at most the begun
 * one).  Queues on the context's stream and makes no synchronisation of its own. */
int fr_dmx_stats_window(fr_dmx* d, uint64_t n_pairs);
/* out[2][n_dest][5]: per mate and destination {reads, bases, quality_bytes, q30_bases, quality_raw_sum}; n_dest
 * as begun.  Synchronises. */
int fr_dmx_stats_get(fr_dmx* d, int n_dest, uint64_t* out);

/* ---- the demux windows' per-cycle statistics (`demux --cycle-stats`; fr_dmx_cycles.hip): where in the read an
 * output is good or bad, per mate, destination and 0-based cycle c, summed over the routed records while they are
 * resident: table mode and sheet mode alike.  A record and its lines are fr_dmx_stats_*'s.  Per record, for every
 * c < len(sequence line) one of six counters gets +1 by the byte's exact value: A, C, G, T, N, other (every other
 * value: lower case and bytes >= 0x80 included); for every c < len(quality line) quality_bytes += 1, q30_bases +=
 * (byte >= 63, unsigned) and quality_raw_sum += byte.  The two lengths are independent.  Cycles at or past
 * max_cycles share one tail bin, index max_cycles.  Summed over the bins, the six base counters are
 * fr_dmx_stats_get's bases, and the three quality fields its own.  Every call below returns FR_ERR_INVALID, with
 * the sums untouched, when the order described is not kept. */
/* Start (or clear) the per-cycle statistics of a demux: n_dest destinations, max_cycles bins and the tail, all sums
 * zero.  Off, and nothing allocated, until this call.  1 <= max_cycles <= 1024, n_dest >= 0. */
int fr_dmx_cycles_begin(fr_dmx* d, int n_dest, int max_cycles);
/* Add the n_pairs record pairs the last fr_dmx_route routed (it found no negative destination; n_pairs must be
 * its count; a window is added once; before the next fr_dmx_load*; that route's n_dest is at most the begun
 * one).  Independent of fr_dmx_tally_window and fr_dmx_stats_window: each may follow one route, once.  Queues on
 * the context's stream and makes no synchronisation of its own. */
int fr_dmx_cycles_window(fr_dmx* d, uint64_t n_pairs);
/* out[2][n_dest][max_cycles + 1][9]: per mate, destination and bin {A, C, G, T, N, other, quality_bytes,
 * q30_bases, quality_raw_sum}; n_dest and max_cycles as begun.  Synchronises. */
int fr_dmx_cycles_get(fr_dmx* d, int n_dest, int max_cycles, uint64_t* out);

/* ---- the demux windows' index mismatch table (`demux -b --barcode-stats`; fr_dmx_bstats.hip): how well the routed
 * pairs' barcodes matched, per destination.  Sheet mode only.  Every R2 record gets one bin byte, bin1 * 5 + bin2:
 * bin k is the number of positions at which the read's index k differs from its reference row's (0, 1, 2, 3 = three
 * or more), or 4 = none.  The reference row of both indexes is the assigned row of a demuxable code; of a hop or an
 * ambiguous code it is the first row within the limit of index 1 and the first within the limit of index 2; an
 * undetermined code has none, and a single-index sheet has no index 2.  The classifier sets the byte of every record
 * it classifies, 255 for every other one (exotic, no '+', length errors); the host sets the bytes of the records it
 * resolves.  Every call below returns FR_ERR_INVALID, with the counts untouched, when the order described is not
 * kept. */
/* Start (or clear) the table of a demux in sheet mode (FR_ERR_INVALID in table mode): n_dest destinations, all
 * counts zero.  Off, nothing allocated and the classifier as it was, until this call; from here on every
 * fr_dmx_load* of mate 1 also leaves the records' bin bytes. */
int fr_dmx_bstats_begin(fr_dmx* d, int n_dest);
/* Set the bin bytes of the given R2 records of the window at hand (the host's resolution of exotic codes, beside
 * fr_dmx_patch).  FR_ERR_INVALID for a record out of range, or with no window loaded since fr_dmx_bstats_begin. */
int fr_dmx_bstats_patch(fr_dmx* d, const uint64_t* recs, const uint8_t* bins, uint64_t n);
/* Count the n_pairs record pairs the last fr_dmx_route routed (it found no negative destination; n_pairs must be
 * its count; a window is counted once; its R2 records were loaded after fr_dmx_bstats_begin; that route's n_dest is
 * at most the begun one).  A bin byte above 24 is not counted.  Independent of the other *_window calls.  Queues on
 * the context's stream and makes no synchronisation of its own. */
int fr_dmx_bstats_window(fr_dmx* d, uint64_t n_pairs);
/* out[n_dest][5][5]: per destination, index-1 bin and index-2 bin the pairs counted; n_dest as begun.
 * Synchronises. */
int fr_dmx_bstats_get(fr_dmx* d, int n_dest, uint64_t* out);

/* ---- the demux windows' validation (`demux --validate`; fr_dmx_validate.hip): are a window's record pairs well
 * formed, and do the mates belong together, checked over the unrouted bytes while they are resident: table mode
 * and sheet mode alike, and nothing of the route is needed.  A record and its lines are fr_dmx_stats_*'s: fr_dmx_records'
 * byte span split at its '\n', absent pieces empty.  Pair k is R1's record k with R2's record k; its violation is
 * the first of these that applies, for R1's record (kinds 1-4), then for R2's (the same four, + 4), then for the
 * pair:
 *   TRUNCATED  the span holds fewer than three '\n' (fewer than four lines);
 *   HEADER     its first byte is not '@';
 *   SEPARATOR  its third piece is empty or does not start with '+';
 *   LENGTH     its second piece (sequence) and fourth piece (quality, without the trailing '\n') differ in length;
 *   NAME       the mates' name tokens differ as bytes: a token is the header line after the '@' up to its first
 *              space or tab (or its end), without its last two bytes when they are "/1" or "/2";
 *   CODE       the text after the last ':' of R1's header line (the whole line without a ':') differs from R2's.
 * The first violation of a window is the one of its lowest pair.  Every call below returns FR_ERR_INVALID, with
 * nothing queued, when the order described is not kept. */
#define FR_DMX_V_TRUNCATED 1
#define FR_DMX_V_HEADER 2
#define FR_DMX_V_SEPARATOR 3
#define FR_DMX_V_LENGTH 4
#define FR_DMX_V_R2 4 /* R2's record kinds are R1's + 4: 5-8 */
#define FR_DMX_V_NAME 9
#define FR_DMX_V_CODE 10
/* Turn the validation on: allocates its result word.  Off, nothing allocated and nothing launched, until this
 * call. */
int fr_dmx_validate_begin(fr_dmx* d);
/* Check the first n_pairs record pairs of the window at hand: after both mates' fr_dmx_load* of the window, once,
 * before the next fr_dmx_load*; n_pairs is at most each mate's record count.  Queues on the context's stream
 * (behind the loads, ahead of the fr_dmx_route that follows) and makes no synchronisation of its own. */
int fr_dmx_validate_window(fr_dmx* d, uint64_t n_pairs);
/* The last queued window's first violation: *first_pair, relative to the window (-1: none), and *kind (0: none).
 * Meant to follow that window's fr_dmx_route, whose read-back has waited for the stream already; synchronises
 * anyway.  FR_ERR_INVALID without a queued window. */
int fr_dmx_validate_result(fr_dmx* d, int64_t* first_pair, int32_t* kind);
/* Free the word and turn the validation off (fr_dmx_destroy does as much). */
int fr_dmx_validate_end(fr_dmx* d);

/* ---- `demux --gz-reader gpu` (fr_dmx_reader.hip): a mate's BGZF file is inflated on the GPU, window by window,
 * into the buffer the window is indexed and routed from; its text reaches the host only through
 * fr_dmx_window_read.  Nothing is allocated and nothing launched before the first fr_dmx_bgzf_open.
 *
 * fr_dmx_bgzf_open: *taken = 1 when the file's first member header is the one fr_bgzf_probe accepts (FLG ==
 * FEXTRA alone, the BC subfield alone); the reader then holds the file and its staging: two pinned buffers of
 * chunk_bytes (0: 32 MiB; at least one member) that a host thread fills ahead with whole members, and their
 * device copy.  A file of any size is taken.  *taken = 0 with FR_OK: not such a file (or not readable: the host
 * reader says why), nothing is held.  The members after the first are walked as the file streams; one that the
 * probe would refuse hands the file over (below) where it stands.
 *
 * fr_dmx_bgzf_fill: the mate's next window.  keep_from: offset in the window at hand of the first byte to keep
 * (0 on the first call: there is none).  The bytes from keep_from on (the carry) move to the front of the
 * mate's other window buffer; whole members are decoded right behind them, each at carry + the decoded sizes
 * before it, while the window holds fewer than `want` bytes and the file has members left (so it ends less
 * than one member, 65536 bytes, past max(carry, want)); every member's status, CRC-32 and size are checked
 * against its trailer and the new bytes must be 7-bit ASCII without '\r' (dmx_text_kernel); then the window is
 * indexed as by fr_dmx_load_device: *n_records, *len.  *eof = 1: no member is left.  The call waits for the
 * context's stream first, so whatever was queued on a window of this mate has read it.
 * Hand-over: when a check fails (or the file cannot be read), *handed_over = 1, nothing of this call's
 * members is delivered: the window is the carry alone (*len its length, no records), *resume is the decoded
 * offset in the file of the first byte not delivered (every byte before it was ASCII without '\r'), and the
 * file is closed: the host reader continues from there.  Otherwise *resume is the decoded offset after this
 * window. */
int fr_dmx_bgzf_open(fr_dmx* d, int mate, const char* path, uint64_t chunk_bytes, int* taken);
int fr_dmx_bgzf_fill(fr_dmx* d, int mate, uint64_t keep_from, uint64_t want, uint64_t* n_records, uint64_t* len,
                     int* eof, int* handed_over, uint64_t* resume);
/* release the mate's file (the buffers stay for the next one); a mate without one: nothing */
int fr_dmx_bgzf_close(fr_dmx* d, int mate);
/* the mate's diagnostics since fr_dmx_create: out[0] files taken, [1] members decoded, [2] fills that delivered
 * a window, [3] hand-overs, [4] the fill (0-based, in its file) at which the last hand-over happened (-1: none),
 * [5] the last fill's inflate-kernel ms, [6] its text-kernel ms, [7] decoded bytes delivered */
int fr_dmx_bgzf_info(fr_dmx* d, int mate, double out[8]);
/* bytes [start, end) of the mate's window at hand, however it was loaded (fr_dmx_load*, fr_dmx_bgzf_fill): for
 * the codes the host resolves, its messages and a hand-over's carry; one copy, whatever the span */
int fr_dmx_window_read(fr_dmx* d, int mate, uint64_t start, uint64_t end, uint8_t* out);

/* ---- GPU deflate over any byte ranges (fr_deflate.hip; fr_dmx_deflate runs it on the routed bytes).
 * Stream s is bytes [offsets[s], offsets[s + 1]) of the device buffer dev_data (4-byte aligned, 16
 * readable bytes past offsets[n_streams]); every stream becomes one raw deflate stream, no larger than
 * zlib level 9 makes it on FASTQ-shaped text (64-KiB blocks, each with a dynamic Huffman code over a
 * cost-minimising parse; a block that would not shrink is stored). */
typedef struct fr_defl fr_defl;
fr_defl* fr_defl_create(int device);
void fr_defl_destroy(fr_defl* z);
const char* fr_defl_last_error(const fr_defl* z);
int fr_defl_run(fr_defl* z, const uint8_t* dev_data, const uint64_t* offsets, int n_streams, uint64_t* comp_bytes,
                uint32_t* crc32);
/* the same over a host buffer (copied to the device first) */
int fr_defl_run_host(fr_defl* z, const uint8_t* data, uint64_t len, const uint64_t* offsets, int n_streams,
                     uint64_t* comp_bytes, uint32_t* crc32);
/* BGZF mode: every stream becomes a run of complete BGZF members (the SAM specification's section 4.1: gzip
 * members whose extra field carries their size, so that a reader finds and inflates them independently).  A
 * stream is cut every 65280 bytes (bgzip's block input); each slice is one final deflate block that
 * references nothing before it, framed by the 18-byte header with BSIZE and the CRC32 / ISIZE trailer.
 * comp_bytes[s] = the run's byte count with its framing, 0 for an empty stream.  No EOF block is produced:
 * the writer of a file appends it once.  A member that would exceed 65536 bytes is never written
 * (FR_ERR_DEVICE; a stored slice makes 65311). */
int fr_defl_run_bgzf(fr_defl* z, const uint8_t* dev_data, const uint64_t* offsets, int n_streams,
                     uint64_t* comp_bytes);
int fr_defl_run_bgzf_host(fr_defl* z, const uint8_t* data, uint64_t len, const uint64_t* offsets, int n_streams,
                          uint64_t* comp_bytes);
/* the last run's kernel times by HIP events (0 when it had no bytes): the block encoder, and the kernel
 * that packs the blocks' outputs (gzip mode's compaction, BGZF mode's framing) */
int fr_defl_kernel_ms(fr_defl* z, double* encode_ms, double* pack_ms);
/* the last run's streams (BGZF mode: member runs), concatenated in stream order */
uint64_t fr_defl_out_bytes(const fr_defl* z);
/* blocks this context stored because their dynamic encoding's bit accounting did not add up (the stored
 * form is always a valid encoding of the block; a nonzero count is a diagnostic, not an error) */
uint64_t fr_defl_stored_fallbacks(const fr_defl* z);
int fr_defl_fetch(fr_defl* z, uint8_t* out, uint64_t len);

/* ---- GPU inflate (fr_inflate.hip): raw deflate streams (RFC 1951) of known decoded size, one wave each.
 * n raw deflate streams: stream s is bytes [in_off[s], in_off[s+1]) of dev_in and must decode to exactly
 * out_off[s+1]-out_off[s] bytes (<= 65536, else FR_ERR_INVALID) at dev_out + out_off[s]. status[s]: 0 or a
 * FR_INFL_* reason; crc32[s]: CRC-32 of the bytes produced (valid when status[s]==0).  Status 0 implies
 * that zlib accepts the same bytes and produces the same output; a stream may be rejected that zlib would
 * take only when it is malformed (an incomplete Huffman code set other than a single distance code).  No
 * input bytes make the decoder read outside its stream or write outside its output range. */
#define FR_INFL_BTYPE 1   /* block type 3 */
#define FR_INFL_STORED 2  /* stored LEN != ~NLEN */
#define FR_INFL_CODELEN 3 /* bad code-length set (over-subscribed, incomplete, bad repeat, no end-of-block code) */
#define FR_INFL_SYMBOL 4  /* invalid literal/length or distance symbol */
#define FR_INFL_DIST 5    /* distance before the start of the output */
#define FR_INFL_INPUT 6   /* input exhausted */
#define FR_INFL_OVERRUN 7 /* the output would overrun its declared size */
#define FR_INFL_SHORT 8   /* output short of its declared size, or input left over */
typedef struct fr_infl fr_infl;
fr_infl* fr_infl_create(int device);
void fr_infl_destroy(fr_infl* z);
const char* fr_infl_last_error(const fr_infl* z);
int fr_infl_run(fr_infl* z, const uint8_t* dev_in, const uint64_t* in_off, uint8_t* dev_out,
                const uint64_t* out_off, int n_streams, uint8_t* status, uint32_t* crc32);
/* the same over a host buffer; the output stays on the device until fr_infl_fetch */
int fr_infl_run_host(fr_infl* z, const uint8_t* data, const uint64_t* in_off, const uint64_t* out_off,
                     int n_streams, uint8_t* status, uint32_t* crc32);
int fr_infl_fetch(fr_infl* z, uint8_t* out, uint64_t len);
/* diagnostics (scripts/inflate_bench.py): the kernel's registers per lane and LDS per workgroup
 * (hipFuncGetAttributes) and the last run's kernel time by HIP events (0 before the first run) */
int fr_infl_kernel_info(fr_infl* z, int* vgprs, int* lds_bytes, double* last_ms);
/* A BGZF file decoded on the GPU as the current file's whole content (between fr_begin_file[_at] with
 * byte_base 0 and fr_end_file; replaces gzip.open(file,"rt") at frender.py:159 for such files).
 * *decoded = 1: every member decoded, its size and CRC-32 equal its trailer, and the bytes went to the
 * tally as fr_feed_device takes them.  *decoded = 0 (FR_OK, nothing fed, context state untouched): the
 * file is not BGZF, a member carries header flags other than FEXTRA or extra subfields besides BC, the
 * file is over the size budget (1 GiB compressed) or its buffers do not fit the device, -s is set, or any
 * member failed -- the caller feeds the file through the host pool,
 * which owns the error behaviour.  *members / *bytes: diagnostics. */
int fr_feed_bgzf(fr_ctx* ctx, const char* path, int* decoded, uint64_t* members, uint64_t* bytes);
/* headers only, no GPU: 1 when fr_feed_bgzf would try the file (every member's FLG is FEXTRA alone and
 * its extra field the BC subfield alone, as bgzip and htslib write them; within the size budget) */
int fr_bgzf_probe(const char* path, uint64_t* members, uint64_t* decoded_bytes);

#ifdef __cplusplus
}
#endif
#endif
