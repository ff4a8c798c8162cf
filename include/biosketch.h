/*
 * biosketch.h -- C ABI of libbiosketch.so, the MI355X (gfx950) k-mer sketching engine.
 *
 * This is the drop-in boundary for the `sketches/` package of shenwei356/bio
 * (reference v0.13.8; file:line below are relative to the reference root).  The
 * reference exposes per-sequence pull iterators; a device cannot be driven one
 * value at a time, so the boundary is "batch in -> all tuples out", and the
 * reference's iterator types become cursors over one read's slice of a result
 * (bindings/go/sketches, bio_amd/csrc/sketches.hpp, bio_amd/sketches.py).
 *
 *   reference constructor / pull method                     ->  bsk_params.kind
 *   NewKmerIterator / NextKmer        iterator.go:668,708   ->  BSK_KMER
 *   NewHashIterator / NextHash        iterator.go:615,658   ->  BSK_NTHASH
 *   NewSimHashIterator / NextSimHash  iterator.go:113,191   ->  BSK_SIMHASH
 *   NewMinimizerSketch / NextMinimizer sketch.go:85,205     ->  BSK_MINIMIZER
 *   NewSyncmerSketch / NextSyncmer    sketch.go:142,312     ->  BSK_SYNCMER
 *   NewProteinIterator / Next         iterator-protein.go:46,76      -> BSK_PROT_HASH
 *   NewProteinMinimizerSketch / Next  sketch-protein.go:62,106       -> BSK_PROT_MINIMIZER
 *   Index()  iterator.go:776 sketch.go:488 iterator-protein.go:93 sketch-protein.go:213
 *                                                           ->  bsk_result pos[] (bit 31 = strand)
 *
 * Plain C: pointers and sizes only, no C++/torch types.  All functions return
 * BSK_OK (0) or a bsk_err; nothing aborts or throws across the boundary.  Host
 * pointers passed in are never retained after the call returns (cgo rule).
 * One bsk_ctx = one GPU + one HIP stream; contexts are independent and may be
 * used from different threads concurrently; a single context is not re-entrant.
 */
#ifndef BIOSKETCH_H
#define BIOSKETCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BSK_ABI_VERSION 1

/* Call-level errors.  1..11 are the reference's sentinel errors, returned when a
 * constructor argument is invalid for EVERY read of the batch
 * (iterator.go:34-53, sketch.go:32-42). */
typedef enum bsk_err {
    BSK_OK = 0,
    BSK_ERR_INVALID_K = 1,     /* ErrInvalidK      iterator.go:34  k < 1 */
    BSK_ERR_EMPTY_SEQ = 2,     /* ErrEmptySeq      iterator.go:37  (declared, never returned upstream) */
    BSK_ERR_SHORT_SEQ = 3,     /* ErrShortSeq      iterator.go:40  (per read: see BSK_ST_SHORT) */
    BSK_ERR_ILLEGAL_BASE = 4,  /* ErrIllegalBase   iterator.go:43  (per read: see BSK_ST_ILLEGAL) */
    BSK_ERR_K_TOO_LARGE = 5,   /* ErrKTooLarge     iterator.go:46 */
    BSK_ERR_INVALID_M = 6,     /* ErrInvalidM      iterator.go:49 */
    BSK_ERR_INVALID_SCALE = 7, /* ErrInvalidScale  iterator.go:52 */
    BSK_ERR_INVALID_S = 8,     /* ErrInvalidS      sketch.go:32 */
    BSK_ERR_INVALID_W = 9,     /* ErrInvalidW      sketch.go:35 */
    BSK_ERR_BUF_NIL = 10,      /* ErrBufNil        sketch.go:38 (declared, never returned upstream) */
    BSK_ERR_BUF_NOT_EMPTY = 11,/* ErrBufNotEmpty   sketch.go:41 (declared, never returned upstream) */
    BSK_ERR_ARG = 64,          /* NULL pointer / inconsistent sizes */
    BSK_ERR_NOMEM = 65,        /* host or device allocation failed */
    BSK_ERR_DEVICE = 66,       /* HIP runtime error; text in bsk_last_error() */
    BSK_ERR_UNSUPPORTED = 67,  /* valid upstream, not implemented here (see DESIGN.md scope) */
    BSK_ERR_NO_DEVICE = 68,    /* no gfx950 device visible: there is NO CPU fallback */
    BSK_ERR_IO = 69,           /* FASTA/Q reader: cannot open / read */
    BSK_ERR_NOT_FASTX = 70,    /* ErrNotFASTXFormat seqio/fastx/reader.go:16 */
    BSK_ERR_BAD_FASTQ = 71,    /* ErrBadFASTQFormat / ErrUnequalSeqAndQual reader.go:19-22 */
    BSK_ERR_STOPPED = 72       /* bsk_pipeline_run: on_chunk returned non-zero and the run was stopped on the consumer's request */
} bsk_err;

typedef enum bsk_kind {
    BSK_KMER = 1,
    BSK_NTHASH = 2,
    BSK_SIMHASH = 3,
    BSK_MINIMIZER = 4,
    BSK_SYNCMER = 5,
    BSK_PROT_HASH = 6,
    BSK_PROT_MINIMIZER = 7
} bsk_kind;

typedef enum bsk_alphabet {
    BSK_ALPHA_DNA = 0,    /* nucleotides (seq.DNAredundant): hashed with ntHash, 2-bit packed on device */
    BSK_ALPHA_PROTEIN = 1,/* seq.Protein: one byte per residue (the `S.Alphabet == seq.Protein`
                             branch of iterator-protein.go:62 / sketch-protein.go:83) */
    /* The other nucleotide alphabets of seq/alphabet.go:352-383.  They are BSK_ALPHA_DNA everywhere but in ONE place: the
     * second strand of NextKmer's two-strand mode comes from RevComInplace (iterator.go:719), which pairs letters with the
     * sequence's OWN alphabet and leaves every other byte as it is (seq/seq.go:386-392):
     *   DNA            acgtACGT <-> tgcaTGCA            RNA            acguACGU <-> ugcaUGCA  (a 'T' stays)
     *   DNAredundant   + ryswkmbdhv <-> yrswmkvhdb      RNAredundant   + ryswkmbdhv <-> yrswmkvhdb
     *   Unlimit        not complemented at all (seq/seq.go:381-383): the second strand is the reversed sequence. */
    BSK_ALPHA_DNA_PLAIN = 2,
    BSK_ALPHA_RNA = 3,
    BSK_ALPHA_RNA_REDUNDANT = 4,
    BSK_ALPHA_UNLIMIT = 5
} bsk_alphabet;

/* Per-read status byte (bsk_result status[]).  Low nibble = what the reference
 * constructor / iterator would have reported for that read; high nibble = flags. */
#define BSK_ST_OK 0x00
#define BSK_ST_SHORT 0x01             /* constructor would return ErrShortSeq; 0 tuples */
#define BSK_ST_ILLEGAL 0x02           /* NextKmer hit ErrIllegalBase (iterator.go:731,746); tuples before it kept */
#define BSK_ST_CODE_MASK 0x0f
#define BSK_ST_FIRST_WINDOW_TIE 0x10  /* the first sorted window (first w k-mer hashes; first 2(k-s) s-mer hashes for
                                         syncmers) holds two equal hashes h[t1] == h[t2], t1 < t2, with nothing smaller
                                         behind t1 inside that window -- the only ties that can sit at buf[0] together,
                                         where upstream's unstable sorts.Quicksort (sketch.go:236,351) may order them
                                         either way; this engine returns the leftmost.  Bit-exactness vs Go is claimed
                                         for reads WITHOUT this flag.  (A tie with a smaller hash behind its first entry
                                         never reaches the front of the buffer while both entries are in it.) */
#define BSK_ST_HAS_NON_ACGT 0x20      /* a byte outside ACGTacgt was hashed (ntHash seed table for such
                                         bytes is unpinned upstream) */

/* reference words of a result (bsk_result_device): (first_tuple << 24) | n_tuples, bit 63 = the read's tuples are 64 apart */
#define BSK_REF_ROWS (1ULL << 63)
#define BSK_REF_FIRST(ref) (((ref) & ~BSK_REF_ROWS) >> 24)
#define BSK_REF_COUNT(ref) ((ref) & 0xffffffULL)
#define BSK_REF_STRIDE(ref) (((ref) & BSK_REF_ROWS) ? 64ULL : 1ULL)

#define BSK_POS_STRAND_BIT 0x80000000u /* pos[] bit 31: 1 iff the reverse-strand hash was the canonical one */
#define BSK_POS_MASK 0x7fffffffu

/* Mirrors the reference constructor arguments 1:1. */
typedef struct bsk_params {
    int32_t kind;       /* bsk_kind */
    int32_t k;          /* k-mer size (all kinds) */
    int32_t w;          /* MINIMIZER / PROT_MINIMIZER: window, sketch.go:85 `w`, sketch-protein.go:62 `w` */
    int32_t s;          /* SYNCMER: s-mer size, sketch.go:142 `s` */
    int32_t m;          /* SIMHASH: m-mer size, iterator.go:113 `m` */
    int32_t scale;      /* SIMHASH: FracMinHash scale, iterator.go:113 `scale` */
    int32_t canonical;  /* KMER / NTHASH / SIMHASH: `canonical` argument (sketches are always canonical) */
    int32_t circular;   /* `circular` argument: first k-1 bases appended (iterator.go:642-646) */
    int32_t codon_table;/* PROT_* on a DNA batch: NCBI genetic-code id for the translation (ignored for protein batches) */
    int32_t frame;      /* PROT_* on a DNA batch: 1,2,3,-1,-2,-3 */
} bsk_params;

typedef struct bsk_ctx bsk_ctx;
typedef struct bsk_batch bsk_batch;
typedef struct bsk_result bsk_result;

/* ---- context ---------------------------------------------------------------- */
int bsk_abi_version(void);
int bsk_device_count(int *n);                      /* number of visible gfx950 devices */
int bsk_ctx_create(int device, bsk_ctx **ctx);     /* hipSetDevice + one stream */
void bsk_ctx_destroy(bsk_ctx *ctx);
int bsk_ctx_sync(bsk_ctx *ctx);                    /* wait for the context's stream */
/* The library's developer switches (environment variables BSK_*, DESIGN.md "Switches") are read ONCE, by bsk_ctx_create -- never on
 * the bsk_sketch path.  A process that changes them afterwards (the test suite does) calls this to have the context read them again. */
int bsk_ctx_reload_options(bsk_ctx *ctx);
/* A test aid, like the entry above: out[0] = the launches whose capped grid the library has sized on this context, out[1] = how many of
 * those got fewer workgroups than their work asked for, so that their grid-stride loops took a later trip (DESIGN.md "Switches",
 * BSK_GRID_CAP).  Counted from bsk_ctx_create on, never reset. */
int bsk_ctx_grid_stats(const bsk_ctx *ctx, uint64_t out[2]);
/* The same for the grids that cap leaves alone -- the persistent waves of the planned sketch kernels and the unit passes beside them:
 * out[0] = the grids sized on this context (its side context included), out[1] = how many of those BSK_UNIT_GRID (DESIGN.md "Switches")
 * gave fewer workgroups than they asked for, so that every wave took several tickets of units.  Counters of their own: the entry above
 * does not see them.  Counted from bsk_ctx_create on, never reset. */
int bsk_ctx_unit_grid_stats(const bsk_ctx *ctx, uint64_t out[2]);
int bsk_build_has_experiments(void);               /* 1 iff built with `make EXPERIMENTS=1`: the measured-and-rejected kernels behind BSK_SEG / BSK_WPR are in */
const char *bsk_last_error(const bsk_ctx *ctx);    /* text of the last BSK_ERR_DEVICE/ARG on this ctx */
const char *bsk_err_name(int err);                 /* "ErrShortSeq", ... (the reference's names) */

/* ---- batches: what a Go caller collects from fastx.Record.Seq.Seq ---------------
 * seqio/fastx/reader.go:229-232 reuses the record buffer, so the shim copies each
 * record's bytes into one contiguous `bytes` array with `offsets[n+1]`.  The call
 * copies to the device and (DNA) packs to 2 bits/base there; host memory is not
 * referenced after return. */
int bsk_batch_from_ascii(bsk_ctx *ctx, const uint8_t *bytes, const uint64_t *offsets, uint64_t n,
                         int alphabet, bsk_batch **out);
/* Pre-packed DNA: words[] holds 16 bases per uint32 (base i of a read in bits
 * [2*(i%16), 2*(i%16)+2) of word i/16, A0 C1 G2 T3); each read starts on a word
 * boundary; desc[r] = (first_word << 24) | n_bases.  n_words = total words. */
int bsk_batch_from_packed(bsk_ctx *ctx, const uint32_t *words, uint64_t n_words,
                          const uint64_t *desc, uint64_t n, bsk_batch **out);
/* Synthetic i.i.d. uniform reads generated ON DEVICE (bench / full-size tests):
 * DNA over ACGT (packed) or protein over ACDEFGHIKLMNPQRSTVWY; counter-based
 * splitmix64(seed, index), so any shard is reproducible. */
int bsk_batch_synth(bsk_ctx *ctx, int alphabet, uint64_t n, uint32_t len, uint64_t seed,
                    bsk_batch **out);
int bsk_batch_info(const bsk_batch *b, uint64_t *n_reads, uint64_t *n_bases, uint64_t *device_bytes,
                   uint64_t *n_non_acgt_reads);
/* Decode reads [first, first+count) back to ASCII on the host (tests: feed the oracle
 * the exact bytes the device hashed).  bytes_cap = capacity of bytes[]; offsets[count+1]. */
int bsk_batch_fetch_ascii(bsk_ctx *ctx, const bsk_batch *b, uint64_t first, uint64_t count,
                          uint8_t *bytes, uint64_t bytes_cap, uint64_t *offsets);
/* DNA/RNA batch -> protein batch on the device: (*seq.Seq).Translate(codon_table, frame, trim=false, clean=false,
 * allowUnknownCodon=true, markInitCodonAsM=false), seq/seq.go:685-708 + seq/codon_tables.go:205-285 -- the call that
 * NewProteinIterator (iterator-protein.go:62-67) and NewProteinMinimizerSketch (sketch-protein.go:83-88) make for
 * non-protein input.  frame: 1,2,3,-1,-2,-3; codon_table: an NCBI genetic-code id of seq/codon_tables.go:431-621.
 * bsk_sketch does this internally when a PROT_* kind is run on a DNA batch (and then applies the constructors'
 * length checks to the NUCLEOTIDE length, as the reference does); this entry point exposes the translation itself. */
int bsk_batch_translate(bsk_ctx *ctx, const bsk_batch *dna, int codon_table, int frame, bsk_batch **out);
/* Host-only: the tables the translate kernel uses for `codon_table` -- [0,4096) amino acid of the codon whose bases
 * are the IUPAC sets (i,j,k) at index i*256+j*16+k ('X' where the reference's 16x16x16 matrix is empty,
 * codon_tables.go:172-174,317-429), [4096,4352) letter -> set (16 = not a base letter, ambiguous_bases.go:28-67),
 * [4352,4416) the 64 plain codons by 2-bit code (A0 C1 G2 T3, first base most significant).  lut_bytes >= 4416. */
int bsk_codon_lut(int codon_table, uint8_t *lut, uint64_t lut_bytes);
void bsk_batch_destroy(bsk_batch *b);

/* ---- FASTA/FASTQ feeding (host side) --------------------------------
 * Record reader with the semantics of seqio/fastx Reader.Read / parseRecord (reader.go:233-471): format from the first
 * non-newline byte, records start at '>' / '@' after a newline, multi-line FASTA and FASTQ, CR dropped, quality lines that
 * start with '@', the reference's edge cases (record without sequence, empty file, newline-only file).  gzip or plain,
 * "-" = stdin.  bsk_fastx_read_chunk returns up to max_records records / stops after max_bytes sequence bytes (0 = no
 * limit; at least one record): concatenated sequence bytes + offsets[n+1], header lines + offsets[n+1], and for FASTQ the
 * concatenated qualities (same offsets as the sequences) -- pointers into reader-owned memory, valid until the next
 * call.  *n == 0 with BSK_OK = end of file.  Errors: BSK_ERR_NOT_FASTX (ErrNotFASTXFormat), BSK_ERR_BAD_FASTQ
 * (ErrBadFASTQFormat / ErrUnequalSeqAndQual), BSK_ERR_IO.  bsk_fastx_info: is_fastq (-1 before the first record) and the
 * alphabet guessed from the first sequence as the reference does, in its order (seq/alphabet.go:413-452): BSK_ALPHA_DNA_PLAIN,
 * BSK_ALPHA_RNA, BSK_ALPHA_DNA (DNAredundant), BSK_ALPHA_RNA_REDUNDANT, BSK_ALPHA_PROTEIN, -1 for "Unlimit".
 * bsk_batch_from_fastx = read_chunk + bsk_batch_from_ascii (alphabet < 0: use the guess). */
typedef struct bsk_fastx bsk_fastx;
int bsk_fastx_open(const char *path, bsk_fastx **out);
int bsk_fastx_read_chunk(bsk_fastx *f, uint64_t max_records, uint64_t max_bytes, uint64_t *n, const uint8_t **seq_bytes,
                         const uint64_t **seq_offsets, const uint8_t **name_bytes, const uint64_t **name_offsets,
                         const uint8_t **qual_bytes);
int bsk_fastx_info(const bsk_fastx *f, int *is_fastq, int *alphabet);
const char *bsk_fastx_error(const bsk_fastx *f);
void bsk_fastx_close(bsk_fastx *f);
int bsk_batch_from_fastx(bsk_ctx *ctx, bsk_fastx *f, uint64_t max_records, uint64_t max_bytes, int alphabet, bsk_batch **out,
                         uint64_t *n_records);

/* Block-parallel reader for PLAIN files (what ChunkChan's producer goroutine, reader.go:562-608, becomes when one thread cannot
 * feed a GPU): the same records in the same order as bsk_fastx_read_chunk, sequences only.  n_threads parser threads work
 * ahead on consecutive byte ranges of `piece_bytes` (0: 8 MiB); each guesses the first record start of its range, runs the
 * record state machine of the serial reader from there, and the consumer (bsk_fastx_par_next, one thread) validates every
 * guess against the previous piece's true end and re-parses a piece that started anywhere else -- so the records are the serial
 * reader's for ANY input (multi-line FASTQ merely runs serially); bsk_fastx_par_info reports how many pieces were re-parsed.
 * BGZF files (bgzip: gzip members of at most 64 KiB that record their own compressed size in a "BC" extra field) are taken too:
 * the members are located without inflating anything, pieces are ranges of the UNCOMPRESSED text, and every parser thread inflates
 * the blocks of its own range.  bsk_fastx_par_open: BSK_ERR_UNSUPPORTED for every other gzip file and for "-" (one serial stream:
 * use bsk_fastx_open), BSK_ERR_NOT_FASTX as above.
 * bsk_fastx_par_next: the next piece with at least one record, *piece == NULL at the end; an error inside a piece is returned
 * by the call after the one that delivered the records before it.  A piece stays valid until bsk_fastx_piece_release (any
 * thread), which must precede bsk_fastx_par_close. */
typedef struct bsk_fastx_par bsk_fastx_par;
typedef struct bsk_fastx_piece bsk_fastx_piece;
int bsk_fastx_par_open(const char *path, int n_threads, uint64_t piece_bytes, bsk_fastx_par **out);
int bsk_fastx_par_next(bsk_fastx_par *f, bsk_fastx_piece **piece);
int bsk_fastx_piece_data(const bsk_fastx_piece *piece, uint64_t *n, const uint8_t **seq_bytes, const uint64_t **seq_offsets);
void bsk_fastx_piece_release(bsk_fastx_par *f, bsk_fastx_piece *piece);
int bsk_fastx_par_info(const bsk_fastx_par *f, int *is_fastq, int *alphabet, uint64_t *reparsed_pieces);
const char *bsk_fastx_par_error(const bsk_fastx_par *f);
void bsk_fastx_par_close(bsk_fastx_par *f);

/* ---- compute -------------------------------------------------------------------
 * Runs the iterator/sketch named by p->kind over every read of the batch.
 * *result == NULL: a result is allocated; otherwise it is reused (bench loops).
 * Output layout (device, SoA, deterministic):
 *   refs[n] u64 = (first_tuple << 24) | n_tuples ; status[n] u8 ; hash[] u64 ; pos[] u32 (bit 31 strand)
 * read r owns tuples first_tuple + j * stride, j = 0 .. n_tuples - 1, in position order -- exactly
 * the sequence of (Next*() value, Index()) pairs the reference iterator yields.  stride is 1, or 64
 * when bit 63 of the reference word (BSK_REF_ROWS) is set: the minimizer / syncmer kernels for short
 * reads write a 64-read unit as ROWS (row j = the j-th tuple of each of the unit's 64 reads), which
 * lets whole rows leave the chip while the reads are still being hashed.
 * BSK_REF_FIRST / BSK_REF_COUNT / BSK_REF_STRIDE decode a reference word.
 * (The tuple arrays contain gaps; use bsk_result_fetch for a dense, rebased CSR copy on the host,
 * bsk_result_compact for one on the device.)
 * KMER / NTHASH / SIMHASH / PROT_HASH emit every position, so pos[] is implicit
 * (NULL): tuple j of read r is position j. */
int bsk_sketch(bsk_ctx *ctx, const bsk_batch *batch, const bsk_params *p, bsk_result **result);

/* Same, repeated: `warmup` untimed runs then `iters` runs, each bracketed by HIP
 * events on the context's stream.  kernel_ms[iters] (may be NULL) receives the
 * per-run duration of the sketch kernel; the call returns after the last run
 * completed.  With *result == NULL one untimed sizing run is done first; with an
 * existing result (from bsk_sketch on the same batch and params) only the
 * warmup + iters launches run.  Used by bench.py (roofline leg).
 * A result of a class plan (bsk_result_class_plan) repeats the lists its own bsk_sketch left in the context: after a later
 * bsk_sketch of another such batch or a bsk_batch_prepare on this context the call returns BSK_ERR_ARG and leaves the
 * result as it was -- call bsk_sketch on it again first. */
int bsk_sketch_timed(bsk_ctx *ctx, const bsk_batch *batch, const bsk_params *p, bsk_result **result,
                     int warmup, int iters, float *kernel_ms);

/* Per-batch preparation a sketch with these parameters would do on its first call, done now (optional; bsk_sketch does it itself and
 * keeps it with the batch): the cut of a class plan (see bsk_result_class_plan), and -- for batches made with BSK_NO_BIN_EARLY=1 -- the
 * LENGTH-BINNED view of a ragged batch of short reads: the kernels walk the 64 reads of a unit in lock-step, so the reads of every chunk
 * of 4096 are grouped by length before units are formed (reference words and status bytes stay at the reads' own positions).  Since
 * round 5 that view is built with the batch (bsk_batch_from_ascii / _from_packed and the refills), in order of length, for whatever
 * parameters come.  *ms (may be NULL) receives the device time of the pass, 0 when the plan needs none.  The
 * reference has no counterpart: its cost is per base of one sequence at a time (sketches/sketch.go:46). */
int bsk_batch_prepare(bsk_ctx *ctx, const bsk_batch *batch, const bsk_params *p, float *ms);

int bsk_result_info(const bsk_result *r, uint64_t *n_reads, uint64_t *n_tuples, int *has_pos);
/* What ran: the name of the kernel the planner launched for this result, as a profiler shows it
 * ("k_minimizer_fast<11,32,true>", "k_syncmer<1>", "... (over tiles)"), its grid and the workgroups (= wavefronts) per CU
 * that grid amounts to.  The string lives as long as the result.  Any out-pointer may be NULL. */
int bsk_result_plan(const bsk_result *r, const char **kernel, int *grid, int *waves_per_cu);
/* Class plans.  The reference sketches one sequence at a time: a long contig costs its own bases, whatever else is in the file
 * (sketch.go:46, :85-94).  A batch whose lengths fall into several classes of the planner (150-base reads + a few of 400 or 5 000
 * bases) is therefore cut by length: the class with most bases runs over the whole batch with the other reads masked, every other class
 * as a batch of its own into the tail of the same result -- callers see one result, bsk_result_plan names every kernel
 * ("k_minimizer_pk<11,false> + k_minimizer_dense<11> [7 reads of 151..400 bases]").  *n_parts = classes besides the bulk (0: one plan),
 * *build_ms = device time of the passes that cut the batch (lists of the other classes' reads + the masked view), paid per bsk_sketch. */
int bsk_result_class_plan(const bsk_result *r, int *n_parts, float *build_ms);
/* Copy reads [first, first+count) to the host.  offsets[count+1] are rebased to 0;
 * hash/pos may be NULL; tuple_cap = capacity (in tuples) of hash[]/pos[]. */
int bsk_result_fetch(bsk_ctx *ctx, const bsk_result *r, uint64_t first, uint64_t count,
                     uint64_t *offsets, uint8_t *status, uint64_t *hash, uint32_t *pos,
                     uint64_t tuple_cap);
/* The status bytes of reads [first, first+count) alone. */
int bsk_result_fetch_status(bsk_ctx *ctx, const bsk_result *r, uint64_t first, uint64_t count, uint8_t *status);
/* The same with narrow side arrays, for streaming callers that move every tuple over the link (bsk_pipeline_*): offsets[count+1] as
 * u32 (scanned on the device: no round trip for the reference words), positions as u16 -- 15 bits + the strand in bit 15
 * (BSK_POS16_STRAND_BIT) -- i.e. 10 bytes per tuple + 5 per read instead of 12 + 17.  BSK_ERR_UNSUPPORTED when a position needs
 * more than 15 bits (reads of 32 768 bases or more) or the range holds 2^32 tuples; *n_tuples (may be NULL) receives the count. */
#define BSK_POS16_STRAND_BIT 0x8000u
#define BSK_POS16_MASK 0x7fffu
int bsk_result_fetch_narrow(bsk_ctx *ctx, const bsk_result *r, uint64_t first, uint64_t count, uint32_t *offsets, uint8_t *status,
                            uint64_t *hash, uint16_t *pos, uint64_t tuple_cap, uint64_t *n_tuples);
/* Dense device copy for device-side consumers (CSR: what bsk_result_fetch delivers to the host, left on the device): offsets[n+1]
 * (u64, offsets[n] = *n_tuples), hash[*n_tuples], pos[*n_tuples] (*pos = NULL for the kinds with implicit positions; pos may be NULL).
 * The arrays belong to the context and stay valid until the next bsk_result_compact on it (or bsk_ctx_destroy).  The reference has no
 * counterpart: its callers collect Next() values into a slice (e.g. sketches/sketch_test.go:93-104). */
int bsk_result_compact(bsk_ctx *ctx, const bsk_result *r, const uint64_t **offsets, const uint64_t **hash, const uint32_t **pos,
                       uint64_t *n_tuples);
/* A result owns its arrays: it stays readable through every entry of this section after its batch was re-filled or
 * destroyed (class plans and tiled calls included: their parts and tile-level results are the library's own).
 * Device pointers (valid until release / next bsk_sketch on this result); refs[] as described above.
 * Long sequences: when a DNA batch holds a sequence longer than the tile threshold (4096 bases, 512 for the every-position kinds; always from 2^24
 * bases on) the engine cuts the sequences into overlapping tiles, runs the same kernels over the tiles and stitches
 * the tile results back (exactly the tuples of the un-tiled iterator).  Such a result is
 * "wide": a sequence can own more than 2^24 tuples, so *refs is NULL and bsk_result_device_wide returns
 * first[n] / count[n] instead (u64 each).  bsk_result_fetch / bsk_result_digest work for both layouts.
 * circular = 1 tiles as well (the sequence with its first k-1 bases appended is one more long sequence), and so do syncmers
 * with s == k (every k-mer with its index, sketch.go:328-331: the w = 1 minimizer).
 * The two-strand k-mer mode (KMER with canonical = 0, iterator.go:713-723) tiles too: forward codes per tile, then the second
 * strand per sequence (the reverse complements of the forward codes, backwards).  Protein kinds on a DNA batch translate a
 * sequence of any length (up to 2^31 bases); the translation is then tiled like any long protein sequence. */
int bsk_result_device(const bsk_result *r, const uint64_t **refs, const uint8_t **status,
                      const uint64_t **hash, const uint32_t **pos);
int bsk_result_device_wide(const bsk_result *r, const uint64_t **first, const uint64_t **count);
/* Order-independent digest computed on device over the whole result:
 *   checksum = sum over tuples of hash * (2*position + 1)   (mod 2^64)
 *   status_counts[k] = number of reads whose status byte has bit pattern k set, for
 *   k in {SHORT, ILLEGAL, FIRST_WINDOW_TIE, HAS_NON_ACGT} (4 entries). */
int bsk_result_digest(bsk_ctx *ctx, const bsk_result *r, uint64_t *checksum, uint64_t *n_tuples,
                      uint64_t status_counts[4]);
/* Frees the result.  Its device arrays (a bench-size result reserves tens of GB) stay with the context for the next result of that context --
 * hipMalloc + hipFree of them cost a hundred kernel times -- up to eight buffers and 40 % of the device memory; the reserve goes back to the
 * device when any allocation of the library runs out of memory, and with bsk_ctx_destroy (BSK_NO_SPARE=1: freed at once). */
void bsk_result_release(bsk_result *r);

/* ---- streaming callers: bounded allocation and the end-to-end pipeline ------------------------
 * bsk_batch_refill_ascii: bsk_batch_from_ascii into an EXISTING batch object (*batch may be NULL the first time): the device
 * buffers are kept and only grow, so a caller that feeds chunk after chunk through one batch per stream allocates nothing in
 * steady state (hipFree synchronises the whole device and would serialise the streams).  The old contents are gone after the
 * call; on error *batch is NULL.  bsk_result_fetch likewise works out of grow-only buffers of its context.
 *
 * bsk_pipeline_fastx / bsk_pipeline_memory: the whole path host bytes -> tuples on the host with its stages overlapped --
 * one producer thread (the role of fastx's ChunkChan goroutine, seqio/fastx/reader.go:562-608) filling pinned chunks of
 * chunk_records records, n_streams workers, each with its own context, doing refill (H2D + pack) -> bsk_sketch ->
 * bsk_result_fetch into pinned memory (fetch_tuples != 0) or only a device digest (fetch_tuples == 0).  It uses nothing but
 * the calls above: a Go host gets the same overlap from one goroutine per stream.  stats->seconds is the wall time from the
 * first read to the last tuple; the per-stage seconds are summed over the workers (they overlap, so they add up to more
 * than `seconds`); checksum is the digest of bsk_result_digest summed over the chunks (positions are per sequence). */
int bsk_batch_refill_ascii(bsk_ctx *ctx, bsk_batch **batch, const uint8_t *bytes, const uint64_t *offsets, uint64_t n, int alphabet);
/* bsk_batch_refill_packed: the same for bsk_batch_from_packed (2-bit words + descriptors prepared on the host: a quarter of the bytes
 * over the link, no pack kernel).  bsk_pipeline_memory packs chunks of pure ACGT reads this way on its worker threads. */
int bsk_batch_refill_packed(bsk_ctx *ctx, bsk_batch **batch, const uint32_t *words, uint64_t n_words, const uint64_t *desc, uint64_t n);
typedef struct bsk_pipeline_stats {
    uint64_t records, bases, tuples, chunks, checksum;
    double seconds;              /* wall */
    double reader_seconds;       /* producer: inside the reader + the copy into pinned memory */
    double reader_wait_seconds;  /* producer: waiting for a free chunk buffer (the device side was the slower one) */
    double h2d_pack_seconds, kernel_seconds, fetch_seconds; /* summed over the workers */
    int32_t n_streams;
    int32_t reader_threads;      /* bsk_pipeline_fastx on a plain file: parser threads of the block-parallel reader (0: serial reader) */
    uint64_t reparsed_pieces;    /* ... and the pieces whose guessed record start was wrong (parsed again, serially) */
    double pin_seconds;          /* summed over all threads: getting the pinned chunk and result buffers (hipHostMalloc, or the pool of earlier runs) */
} bsk_pipeline_stats;
int bsk_pipeline_fastx(int device, const char *path, int alphabet /* -1: guess from the first record */, const bsk_params *p, int n_streams,
                       uint64_t chunk_records, int fetch_tuples, bsk_pipeline_stats *stats);
int bsk_pipeline_memory(int device, const uint8_t *bytes, const uint64_t *offsets, uint64_t n, int alphabet, const bsk_params *p,
                        int n_streams, uint64_t chunk_records, int repeat, int fetch_tuples, bsk_pipeline_stats *stats);
/* The same over SEVERAL GPUs of one node (devices[n_devices]; a device may be named more than once): one producer side, n_streams workers
 * per device, every worker takes the next chunk from the one queue -- the role of ChunkChan feeding W workers
 * (seqio/fastx/reader.go:562-608) with the workers spread over the node's GPUs.  Reads are independent: nothing crosses between devices,
 * and the statistics (records, tuples, the order-independent checksum) are the whole job's. */
int bsk_pipeline_fastx_multi(const int *devices, int n_devices, const char *path, int alphabet, const bsk_params *p, int n_streams,
                             uint64_t chunk_records, int fetch_tuples, bsk_pipeline_stats *stats);
int bsk_pipeline_memory_multi(const int *devices, int n_devices, const uint8_t *bytes, const uint64_t *offsets, uint64_t n, int alphabet,
                              const bsk_params *p, int n_streams, uint64_t chunk_records, int repeat, int fetch_tuples, bsk_pipeline_stats *stats);
/* Several files through ONE pipeline, n_readers of them (0: min(n_paths, 8)) read at the same time, each by its own producer thread --
 * the block-parallel reader for a plain file, the serial one for a gzip file (one zlib stream per file is how gzip input scales).
 * A file is closed as soon as its last chunk is on the device.  The statistics are those of the whole job. */
int bsk_pipeline_fastx_files(int device, const char *const *paths, int n_paths, int alphabet, const bsk_params *p, int n_streams, int n_readers,
                             uint64_t chunk_records, int fetch_tuples, bsk_pipeline_stats *stats);

/* ---- the pipeline with a consumer ----------------------------------------------------------------------------------------------
 * What fastx's ChunkChan is to the reference's callers (seqio/fastx/reader.go:562-608: every chunk of records, in input order, handed to
 * whoever ranges over the channel) with the sketching done on the way: open a pipeline over a source, then
 *     for (;;) { bsk_pipeline_next(pl, &c); if (!c) break;  ... use c ...;  bsk_pipeline_release(pl, c); }   bsk_pipeline_close(pl, &stats);
 * Chunks arrive in the order the producer queued them (= record order for one source); a chunk's arrays live in pinned host memory of the
 * pipeline until the chunk is released (the pool of output buffers is bounded: a consumer that holds 2 * workers + 2 chunks stalls the run).
 * sink selects what crosses the link for every chunk:
 *   BSK_SINK_TUPLES  every tuple, as bsk_result_fetch_narrow delivers it (offsets32 / pos16; offsets64 / pos32 when a chunk holds a read
 *                    of 32 768 bases or more, or 2^32 tuples) -- record i of the chunk owns hash[offsets[i] .. offsets[i+1]) in Next() order;
 *   BSK_SINK_SETS    the on-device reduction of bsk_result_sets: per record the ascending distinct hash values with hash <= MaxUint64 /
 *                    sets_scale (iterator.go:181-185; sets_scale <= 1: no filter) -- offsets32 + hash, n_values values;
 *   BSK_SINK_COUNTS  nothing but the counts and the device-side digest (bsk_result_digest) in `checksum`.
 * host_checksum != 0: the worker also folds what it fetched into `checksum` (tuples: the order-independent sum of bsk_result_digest; sets:
 * the sum of the values) -- the statistics-only entry points bsk_pipeline_fastx / _memory use this.
 * bsk_pipeline_next blocks until the next chunk is ready; *chunk == NULL with BSK_OK is the end of the input.  One consumer thread at a
 * time.  bsk_pipeline_close may be called at any point (it stops the run) and frees the pipeline; stats may be NULL. */
typedef struct bsk_pipeline bsk_pipeline;
enum { BSK_SINK_COUNTS = 0, BSK_SINK_TUPLES = 1, BSK_SINK_SETS = 2 };
typedef struct bsk_pipeline_config {
    const int *devices;      /* the GPUs of the run (a device may be named more than once) */
    int32_t n_devices;
    int32_t n_streams;       /* workers (context + HIP stream) per device */
    uint64_t chunk_records;  /* records per chunk (0: the reader's default) */
    int32_t sink;            /* BSK_SINK_* */
    int32_t sets_scale;      /* BSK_SINK_SETS: FracMinHash scale */
    int32_t alphabet;        /* bsk_alphabet, -1: guess from the first record (files) */
    int32_t host_checksum;
    int32_t n_readers;       /* several files: how many are read at the same time (0: min(n_paths, 8); chunk order = queue order) */
    int32_t reserved;
} bsk_pipeline_config;
typedef struct bsk_chunk {
    uint64_t sequence;       /* 0, 1, 2 ...: the delivery order */
    int32_t source_index;    /* which of the run's files */
    int32_t device;          /* the GPU that sketched it */
    uint64_t first_record;   /* index of the chunk's first record in its source */
    uint64_t n_records, n_bases, n_tuples;
    uint64_t n_values;       /* entries of hash[]: n_tuples (TUPLES), distinct filtered values (SETS), 0 (COUNTS) */
    uint64_t checksum;
    uint64_t link_bytes;     /* bytes this chunk's output moved device -> host */
    int32_t sink, has_pos;
    const uint32_t *offsets32; /* [n_records + 1], or NULL when offsets64 is set */
    const uint64_t *offsets64;
    const uint8_t *status;     /* [n_records] BSK_ST_* */
    const uint64_t *hash;
    const uint16_t *pos16;     /* TUPLES with positions: BSK_POS16_* encoding; NULL for implicit positions / SETS / when pos32 is set */
    const uint32_t *pos32;
    void *opaque;
} bsk_chunk;
int bsk_pipeline_open_fastx(const bsk_pipeline_config *cfg, const char *const *paths, int n_paths, const bsk_params *p, bsk_pipeline **out);
int bsk_pipeline_open_memory(const bsk_pipeline_config *cfg, const uint8_t *bytes, const uint64_t *offsets, uint64_t n, int repeat,
                             const bsk_params *p, bsk_pipeline **out);
int bsk_pipeline_next(bsk_pipeline *pl, const bsk_chunk **chunk);
int bsk_pipeline_release(bsk_pipeline *pl, const bsk_chunk *chunk);
int bsk_pipeline_close(bsk_pipeline *pl, bsk_pipeline_stats *stats);
const char *bsk_pipeline_error(const bsk_pipeline *pl);
/* Stops the run from ANY thread without freeing anything: a consumer blocked in bsk_pipeline_next (and every later call) returns -1, the
 * workers wind down.  What a host with a consumer thread of its own (Go: the goroutine behind Pipeline.Chunks(), the role of fastx's
 * ChunkChan goroutine, reader.go:562-608) calls BEFORE it joins that thread and closes: bsk_pipeline_close frees the pipeline and must
 * not overlap with a bsk_pipeline_next. */
int bsk_pipeline_cancel(bsk_pipeline *pl);
/* next / on_chunk / release until the end (or until on_chunk returns non-zero: BSK_ERR_STOPPED), then close: the callback form of the
 * loop above. */
typedef int (*bsk_chunk_fn)(void *user, const bsk_chunk *chunk);
int bsk_pipeline_run(bsk_pipeline *pl, bsk_chunk_fn on_chunk, void *user, bsk_pipeline_stats *stats);

/* The pipelines keep their pinned host buffers in a process-wide pool between calls (pinning is the start-up cost of a run:
 * pin_seconds); this returns the pooled memory to the system.  Safe at any time; buffers of a running pipeline are not affected. */
void bsk_pipeline_trim(void);

/* ---- multi-GPU: the one collective of the path ----------------------------
 * Reads shard by record; no tuple ever crosses GPUs.  What a job gathers at its end is a handful of u64 counters per GPU
 * (reads, bases, tuples, flagged reads ...): one all_gather over RCCL (xGMI inside a node), 8 * n_counters bytes per rank.
 * librccl is opened on first use; a single-GPU caller never loads it.
 *   one process (or thread) per GPU:  rank 0 calls bsk_comm_unique_id and hands the 128 bytes to the other ranks by whatever
 *     channel the host has (the job launcher's store, a Go channel); every rank then calls bsk_comm_init_rank on its own
 *     context and bsk_gather_counts after its work;
 *   one thread driving several contexts (a Go host with one goroutine per GPU that joins before reporting):
 *     bsk_comm_init_all once, bsk_gather_counts_all after the work -- mine[n][n_counters] in rank order, all[n][n_counters]
 *     as every rank received it (checked to be identical).
 * all[] is world * n_counters values in rank order.  The calls block until the data is on the host. */
#define BSK_UNIQUE_ID_BYTES 128
#define BSK_MAX_COUNTERS 16
int bsk_comm_unique_id(uint8_t *id /* [BSK_UNIQUE_ID_BYTES] */);
int bsk_comm_init_rank(bsk_ctx *ctx, const uint8_t *id, int rank, int world);
int bsk_comm_init_all(bsk_ctx *const *ctxs, int n);
int bsk_gather_counts(bsk_ctx *ctx, const uint64_t *mine, int n_counters, uint64_t *all);
int bsk_gather_counts_all(bsk_ctx *const *ctxs, int n, const uint64_t *mine, int n_counters, uint64_t *all);
void bsk_comm_destroy(bsk_ctx *ctx);

/* ---- sketch sets ----------------------------------------------------
 * The distinct hash values of a result in ascending order -- what the reference's consumers (kmcp, unikmer) build from
 * the Next() stream of a sketch and keep on disk: collect, sort, de-duplicate.  scope: one set per sequence or one set
 * for the whole batch.  scale > 1: FracMinHash, keep hash <= MaxUint64/scale (the rule of iterator.go:181-185).
 * Computed on the device (rocPRIM segmented radix sort + scan); offsets[n_sets+1] and values[] stay there until
 * bsk_sets_release.  At most 2^32 values per call. */
typedef struct bsk_sets bsk_sets;
enum { BSK_SETS_PER_SEQUENCE = 0, BSK_SETS_WHOLE_BATCH = 1 };
int bsk_result_sets(bsk_ctx *ctx, const bsk_result *r, int scope, int scale, bsk_sets **out);
/* The result slot.  The entries below that take bsk_sets **out / **sets, bsk_hits **hits / **top or bsk_compare **cmp read the slot as
 * well as write it: it holds NULL (the entry makes a new object) or the object of an earlier call on the same context, whose device
 * arrays are kept and only grow.  Every such entry works in two steps.  What it checks BEFORE it takes the object over fails with the
 * slot as it was: the object is still the caller's, its contents intact.  Then the object is the entry's -- from here any failure
 * releases it and leaves the slot NULL, and BSK_OK stores it back.  Which error falls on which side:
 *   bsk_sets_op, _op_counted, _reduce, _filter_counts, _bottom, bsk_index_search and bsk_index_search_counted: every BSK_ERR_ARG and
 *     the 2^32 limits (BSK_ERR_UNSUPPORTED) keep the slot; BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_hits_top: every BSK_ERR_ARG keeps the slot; its BSK_ERR_UNSUPPORTED (a sort key beyond 63 bits, known after a read-back),
 *     BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_sets_compare, _compare_counted: every BSK_ERR_ARG keeps the slot; both size limits (BSK_ERR_UNSUPPORTED) are checked after the
 *     object is taken over and release it, as BSK_ERR_NOMEM and BSK_ERR_DEVICE do.
 *   bsk_sets_neighbors, _neighbors_counted: as bsk_sets_compare -- every BSK_ERR_ARG keeps the slot, its size limits
 *     (BSK_ERR_UNSUPPORTED), BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_hits_cluster (bsk_clusters **out) and bsk_hits_from_host: every BSK_ERR_ARG and the 2^32 limits keep the slot; BSK_ERR_NOMEM and
 *     BSK_ERR_DEVICE release.
 *   bsk_hits_fold: every BSK_ERR_ARG -- a row that is not strictly ascending and a target beyond the last group included, which one
 *     small device pass finds before the object is taken over -- and the 2^32 limits keep the slot; BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_hits_filter, bsk_hits_top_by: every BSK_ERR_ARG -- a target beyond the target norms and a denominator that is not positive
 *     included, which one small device pass finds before the object is taken over -- and the 2^32 limits keep the slot; BSK_ERR_NOMEM
 *     and BSK_ERR_DEVICE release.
 *   bsk_hits_transpose, bsk_hits_tally (bsk_tally **out): every BSK_ERR_ARG -- a target >= n_targets included, which one small device
 *     pass finds before the object is taken over, and for the tally a flag bit and a table of another n_targets -- and the 2^32 limits
 *     keep the slot; BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_hits_merge: every BSK_ERR_ARG -- a duplicate without BSK_MERGE_ADD included, which the device passes find before the object is
 *     taken over -- and every BSK_ERR_UNSUPPORTED -- the 2^32 limits and a target_base + target beyond 32 bits -- keep the slot;
 *     BSK_ERR_NOMEM and BSK_ERR_DEVICE release.
 *   bsk_result_sets_windows: as bsk_sets_compare -- every BSK_ERR_ARG keeps the slot; both 2^32 limits (BSK_ERR_UNSUPPORTED: the windows in
 *     total, the gathered tuples), known after a read-back, release it, as BSK_ERR_NOMEM and BSK_ERR_DEVICE do.
 *   bsk_result_sets_reuse, _counted: a NULL `sets` and sets of another context (BSK_ERR_ARG) keep the slot.  Every other error releases:
 *     a NULL r, a bad scope, a bad scale and a result of another context (BSK_ERR_ARG all four), the 2^32 limit, memory, the device.
 * bsk_result_sets, bsk_sets_from_host and bsk_index_build only write their slot: it is NULL after an error, whatever it held
 * (bsk_result_sets: after any error but a NULL argument, which leaves it untouched).
 *
 * bsk_result_sets into an existing object (*sets may be NULL the first time): the device arrays are kept and only grow -- a streaming
 * caller allocates nothing in steady state.  Sets of another context are refused and stay in the slot; on every other error the object
 * is released and *sets is NULL. */
int bsk_result_sets_reuse(bsk_ctx *ctx, const bsk_result *r, int scope, int scale, bsk_sets **sets);
/* All sets to the host in narrow form: u32 offsets[n_sets + 1] (narrowed on the device) + the values, copied on the context's stream
 * (4 bytes per set + 8 per value over the link). */
int bsk_sets_fetch_narrow(bsk_ctx *ctx, const bsk_sets *s, uint32_t *offsets, uint64_t *values, uint64_t value_cap);
int bsk_sets_info(const bsk_sets *s, uint64_t *n_sets, uint64_t *n_values);
/* Sets first .. first + count - 1 to the host: offsets[count + 1] rebased to 0, then their values (values may be NULL: offsets only).
 * BSK_ERR_ARG for a range outside the sets, for more values than value_cap, and -- like bsk_sets_fetch_narrow -- for sets that belong to
 * another context. */
int bsk_sets_fetch(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *offsets, uint64_t *values,
                   uint64_t value_cap);
int bsk_sets_device(const bsk_sets *s, const uint64_t **offsets, const uint64_t **values);
void bsk_sets_release(bsk_sets *s);

/* ---- set algebra on sketch sets ----------------------------------------------------
 * bsk_sets_op: out[i] = a[i] op b[i] when b holds as many sets as a; when b holds exactly one set (and a any other number) every
 * set of a is combined with that one set (broadcast: masking a host set out of every read set).  Anything else is BSK_ERR_ARG, as
 * is an unknown op.  The output has a's number of sets, strictly ascending inside a set, and is an ordinary bsk_sets of ctx:
 * index it, search it, fetch it.  a == b (the same object) is legal.  *out: NULL, or the object of an earlier bsk_sets_op /
 * bsk_sets_reduce on this context, whose device arrays are kept and only grow; *out == a or *out == b is BSK_ERR_ARG.  Which error
 * keeps *out and which releases it: "The result slot" above.  a and b must
 * belong to ctx.  Inputs that hold 2^32 values or more together are BSK_ERR_UNSUPPORTED.  Any u64 is a legal value, 0 and 2^64-1
 * included.  A merge, not a sort: pairs of few values take a group of 16 lanes, larger ones a wavefront, and beyond one
 * wavefront's LDS the merged sequence is cut into tiles that spread over the device (bsk_sets_plan counts the pairs per path). */
enum { BSK_SETOP_UNION = 0, BSK_SETOP_INTERSECT = 1, BSK_SETOP_DIFF = 2 /* a \ b */, BSK_SETOP_SYMDIFF = 3 };
int bsk_sets_op(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets **out);

/* bsk_sets_reduce: the groups are runs of consecutive sets of s -- group g is sets group_offsets[g] .. group_offsets[g + 1] - 1;
 * group_offsets[0] == 0, non-decreasing, group_offsets[n_groups] == the number of sets of s, else BSK_ERR_ARG (checked on the
 * host, nothing kept).  Output set g holds the values that occur in at least min_members of the group's member sets: 1 is the
 * union, BSK_MEMBERS_ALL the intersection over every member (empty members included: one empties it), any other m keeps the
 * values of >= m members (a group of fewer members yields the empty set); 0 is BSK_ERR_ARG.  An empty group yields an empty set.
 * *out as in bsk_sets_op; *out == s is BSK_ERR_ARG.  The host pointer is not retained. */
#define BSK_MEMBERS_ALL 0xFFFFFFFFu
int bsk_sets_reduce(bsk_ctx *ctx, const bsk_sets *s, const uint64_t *group_offsets /* host, [n_groups+1] */,
                    uint64_t n_groups, uint32_t min_members, bsk_sets **out);

/* what made these sets: a short description, and how many pairs of the last bsk_sets_op into s took the group, wave and tiled
 * path; sets made by any other call report an empty string and zeros */
int bsk_sets_plan(const bsk_sets *s, const char **plan, uint64_t n_by_path[3]);  /* either out-pointer may be NULL */

/* ---- containment search of sets against a device-resident index ----------------------------------------------------
 * What a kmcp-style consumer does with the sets: for every query set (a read, a genome), which target sets share how many values
 * with it -- containment shared / |q|, Jaccard shared / (|q| + |t| - shared) -- computed where the sets already are.
 *
 * Sets from the host (e.g. a reference collection loaded from disk): offsets[n_sets+1] (offsets[0] = 0, non-decreasing),
 * values[offsets[n_sets]], strictly ascending inside every set -- anything else is BSK_ERR_ARG (checked; nothing is kept on error).
 * Any u64 is a legal value, 0 and 2^64-1 included.  The result is an ordinary bsk_sets of ctx: bsk_sets_info / _fetch / _device /
 * _release work on it.  Host pointers are not retained. */
int bsk_sets_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values, bsk_sets **out);

/* Inverted index of a collection of target sets: value -> ascending list of the targets that hold it.  It owns copies of everything
 * it needs (the target sets' sizes included), so the bsk_sets may be released after the build.  Layout: the values pass a bijective
 * 64-bit mixer (the splitmix64 finalizer), the distinct mixed keys are sorted, each with its posting list of target ids (u32), and a
 * directory over the top b bits of the mixed key (2^b <= distinct keys < 2^(b+1)) points into the keys: a bucket holds one or two
 * keys on average, and a lookup reads one directory entry and scans its whole bucket.  Fewer than 2^32 targets and fewer than
 * 2^32 postings (values over all targets), else BSK_ERR_UNSUPPORTED.  max_bucket: the most keys one directory bucket holds. */
typedef struct bsk_index bsk_index;
int bsk_index_build(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out);
int bsk_index_info(const bsk_index *ix, uint64_t *n_targets, uint64_t *n_postings, uint64_t *n_distinct, uint64_t *max_bucket,
                   uint64_t *device_bytes); /* any out-pointer may be NULL */
void bsk_index_release(bsk_index *ix);

typedef struct bsk_search_params {
    uint32_t min_shared;    /* 0 is taken as 1: a pair that shares nothing is never listed */
    uint32_t reserved;      /* 0 */
    double min_query_cov;   /* 0..1 */
    double min_target_cov;  /* 0..1 */
} bsk_search_params;
/* For every query set q and target t with s = |q & t|: the pair is listed iff
 *   s >= max(min_shared, 1)  &&  (double)s >= min_query_cov * (double)|q|  &&  (double)s >= min_target_cov * (double)|t|
 * (IEEE double, exactly this expression).  Hits are CSR by query: offsets[n_queries+1] (u64), target[] (u32) ascending inside a
 * query, shared[] (u32).  *hits may be NULL (new object) or the object of an earlier search on this context: its device arrays are
 * kept and only grow (as bsk_result_sets_reuse); an argument error and the 2^32 limits leave *hits as it was, a memory or device
 * error releases it and sets *hits to NULL ("The result slot" above).  queries and ix must belong to ctx.
 * Everything runs on the context's stream; the host reads back sizes only.  A query whose posting lists hold more target ids than
 * one wavefront's LDS budget takes an exact sort-based path instead (bsk_hits_plan counts them). */
typedef struct bsk_hits bsk_hits;
int bsk_index_search(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits);
int bsk_hits_info(const bsk_hits *h, uint64_t *n_queries, uint64_t *n_hits);
/* what the last search into h ran: a short description, and how many queries took the large-query path (either may be NULL) */
int bsk_hits_plan(const bsk_hits *h, const char **plan, uint64_t *n_large_queries);
int bsk_hits_fetch(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint64_t *offsets /* rebased */, uint32_t *target,
                   uint32_t *shared, uint64_t hit_cap);
int bsk_hits_device(const bsk_hits *h, const uint64_t **offsets, const uint32_t **target, const uint32_t **shared);
void bsk_hits_release(bsk_hits *h);

/* ---- classifying reads: an index several contexts search, the n best hits of a query, the pipeline's hits sink ------------------
 * A handle on ix for another context.  Same device as ix: the device arrays are shared (reference counted, read-only);
 * another device: the arrays are copied there once.  The handle is searched with bsk_index_search(ctx, handle, ...) and
 * released with bsk_index_release; a device's arrays go when their last handle goes, in any release order (the index
 * bsk_index_build returned is one handle among the others: it may be released while attached handles live).
 * bsk_index_info works on a handle and reports the same numbers.  A handle may be attached from a handle.
 * The index is read-only during a search and every scratch array is the searching context's own, so several contexts may
 * search their handles of one index at the same time from several threads.  A release must not overlap a search ON THAT
 * SAME HANDLE (nor an attach from it); releases and searches of different handles need no ordering. */
int bsk_index_attach(bsk_ctx *ctx, const bsk_index *ix, bsk_index **handle);

/* For every query of h the min(n, its hit count) hits with the largest shared count (for one query that is the order of
 * containment shared/|q|), ties by ascending target id; inside a query they are stored in that order (NOT ascending by
 * target as bsk_index_search stores them).  *top: NULL or the object of an earlier call on this context (arrays kept,
 * grow only; errors: "The result slot" above); *top == h is BSK_ERR_ARG.  n == 0 is BSK_ERR_ARG.  The result is an
 * ordinary bsk_hits: _info / _fetch / _device / _release work on it; bsk_hits_plan describes what ran (queries of at most
 * 16 hits: a group of 16 lanes each; more hits and n <= 16: n rounds of a wave-wide maximum; n > 16: a sort in LDS up to
 * 1 024 hits, beyond that one device-wide key sort -- bsk_hits_plan's count is the queries of that last path).
 * Everything runs on the context's stream; the host reads back one block of sizes.  The key of the sort path holds
 * (queries on that path) x (largest shared count) x (most hits of one query): beyond 63 bits -- far past what device
 * memory holds -- the call is BSK_ERR_UNSUPPORTED. */
int bsk_hits_top(bsk_ctx *ctx, const bsk_hits *h, uint32_t n, bsk_hits **top);

/* BSK_SINK_HITS: reads in, the best targets of every read out.  Per chunk a worker sketches, reduces the result to per-record sets
 * (bsk_result_sets_reuse, cfg->sets_scale), searches them on its own handle of s->index (bsk_index_search with s->params) and, for
 * top_n != 0, keeps every read's top_n best (bsk_hits_top); the sets never leave the device.  A chunk's offsets32 (offsets64 from 2^32
 * hits) are the records' hit offsets, n_values the number of hits, hash == NULL; bsk_chunk_hits gives target[] and shared[] (valid
 * until the chunk is released).  link_bytes is n_records * 5 + n_hits * 8 in the narrow form; with host_checksum, checksum is the sum
 * of target + shared over the hits.  next / release / close / cancel / run, the record order, status[] and the statistics are those of
 * the other sinks.  cfg->sink must be BSK_SINK_HITS for these two entries, and BSK_SINK_HITS is BSK_ERR_ARG in bsk_pipeline_open_fastx
 * / _memory.  s->index may belong to any context and any device: the pipeline attaches a handle per worker (one copy per further
 * device) and releases them when it closes; the caller may release s->index only after bsk_pipeline_close.
 * The index must have been built from sets of the same bsk_params and the same scale as p and cfg->sets_scale: the pipeline cannot
 * check that, and hits against an index of other parameters are meaningless. */
enum { BSK_SINK_HITS = 3 };
typedef struct bsk_pipeline_search {
    const bsk_index *index;     /* of any context; the pipeline attaches a handle per worker (one copy per further device) */
    bsk_search_params params;
    uint32_t top_n;             /* 0: every hit, targets ascending; n: bsk_hits_top order */
    uint32_t reserved;          /* 0 */
} bsk_pipeline_search;
int bsk_pipeline_open_fastx_search(const bsk_pipeline_config *cfg, const char *const *paths, int n_paths, const bsk_params *p,
                                   const bsk_pipeline_search *s, bsk_pipeline **out);
int bsk_pipeline_open_memory_search(const bsk_pipeline_config *cfg, const uint8_t *bytes, const uint64_t *offsets, uint64_t n, int repeat,
                                    const bsk_params *p, const bsk_pipeline_search *s, bsk_pipeline **out);
/* BSK_SINK_HITS chunks: offsets32 / offsets64 are the records' hit offsets, n_values the number of hits, hash == NULL */
int bsk_chunk_hits(const bsk_chunk *c, const uint32_t **target, const uint32_t **shared);

/* ---- counted sketch sets: abundance on the device ----------------------------------------------------
 * A counted set is an ordinary bsk_sets plus a device array counts[n_values] (u32) parallel to values: how often the value occurred.
 * Every other entry treats such an object as its values only; an entry that writes into a re-used counted object leaves it uncounted
 * (the array is kept, like the others).
 * bsk_result_sets_counted: scope, scale, the 2^32 limit and the *sets rules of bsk_result_sets_reuse (*sets may be NULL; arrays kept,
 * grow only; sets of another context stay in the slot, any other error releases the object and *sets is NULL); offsets and values are those of bsk_result_sets, counts[i] is the
 * number of tuples of the set's scope -- the sequence, or the whole batch -- that hold values[i].  Values above MaxUint64 / scale are
 * neither kept nor counted. */
int bsk_result_sets_counted(bsk_ctx *ctx, const bsk_result *r, int scope, int scale, bsk_sets **sets);
int bsk_sets_counts_device(const bsk_sets *s, const uint32_t **counts);            /* *counts = NULL for an uncounted object */
/* the counts of sets first .. first + count - 1 (range and cap rules of bsk_sets_fetch); BSK_ERR_ARG for an uncounted object */
int bsk_sets_fetch_counts(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint32_t *counts, uint64_t count_cap);
/* bsk_sets_from_host with counts[offsets[n_sets]]; a count of 0 is BSK_ERR_ARG (nothing is kept) */
int bsk_sets_from_host_counted(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_sets, const uint64_t *values,
                               const uint32_t *counts, bsk_sets **out);
/* bsk_sets_op_counted: the values of ADD / KEEP / DROP are the union / intersection / difference of bsk_sets_op.  ADD: count
 * ca + cb, saturating at 2^32 - 1; KEEP: the values of a that b holds, with a's counts; DROP: those b does not hold, with a's counts.
 * An uncounted operand counts 1 for every value; the output is always counted.  Pairing as bsk_sets_op, and besides an a of exactly
 * one set against a b of n sets yields n sets, a op b[i] (one sample against every genome).  *out, errors, a == b and the 2^32 limit
 * as bsk_sets_op; bsk_sets_plan reports the pairs per path. */
enum { BSK_COUNTOP_ADD = 0, BSK_COUNTOP_KEEP = 1, BSK_COUNTOP_DROP = 2 };
int bsk_sets_op_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, int op, bsk_sets **out);
/* the values with min_count <= count <= max_count, and their counts; s must be counted; min_count == 0 or min_count > max_count is
 * BSK_ERR_ARG; *out as in bsk_sets_reduce */
int bsk_sets_filter_counts(bsk_ctx *ctx, const bsk_sets *s, uint32_t min_count, uint32_t max_count, bsk_sets **out);
/* per set of the range the sum of its counts (u64: exact); an uncounted object gives the sets' sizes */
int bsk_sets_totals(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *totals /* host */);

/* ---- MinHash: bottom-n sets, all-pairs comparison ----
 * bsk_sets_bottom: out[i] is the min(n, |s[i]|) smallest values of s[i] -- the fixed-size (Mash, sourmash num=) sketch; the sets are
 * ascending, so these are a prefix.  A counted input yields a counted output with the counts of the kept values, an uncounted input an
 * uncounted output.  n == 0 is BSK_ERR_ARG.  *out as in bsk_sets_reduce: NULL, or the object of an earlier op on this context (arrays
 * kept, grow only); *out == s is BSK_ERR_ARG; an argument error leaves *out as it was, a memory or device error releases it and sets
 * *out to NULL.  The result is an ordinary bsk_sets: index it, search it, fetch it, use it in the algebra.
 *
 * bsk_sets_compare: for every pair (i, j), i < n_a, j < n_b, walk the distinct values of a[i] | b[j] in ascending order and stop after
 * `limit` of them (limit == 0: never stop early).  total[i * n_b + j] is the number walked, min(limit, |a[i] | b[j]|);
 * shared[i * n_b + j] is how many of the walked values both sets hold.  Both are dense row-major u32 matrices on the device.
 *   limit == 0: shared is |a & b| and total is |a | b| -- the exact Jaccard shared / total;
 *   limit == n: shared / total is the Mash estimator of the Jaccard from bottom-n sketches;
 *   only the `limit` smallest values of each set can take part, so the result on full sets equals the result on their
 *   bsk_sets_bottom(limit).
 * Any u64 is a legal value, 0 and 2^64-1 included.  a == b (the same object) is legal; the full matrix is computed.  n_a == 0 or
 * n_b == 0 gives an empty result with BSK_OK.  a and b must belong to ctx.  Inputs that together hold 2^32 values or more (a == b:
 * counted once), or more than 2^31 cells, are BSK_ERR_UNSUPPORTED; both are checked before any device memory is allocated.  *cmp: NULL, or the
 * object of an earlier compare on this context, whose device arrays are kept and only grow; an argument error leaves *cmp as it was,
 * any other error -- the two limits included -- releases it and sets *cmp to NULL ("The result slot" above).  Everything runs on the context's stream;
 * the host reads back one block of figures.
 * Which route for an all-against-all: this one is dense -- its cost is the cells times the values a pair walks, whatever the sets
 * share -- and is the only one that gives the limit-bounded (Mash) numbers; it suits sketches of up to a few thousand values.
 * bsk_index_build + bsk_index_search is output-sparse -- its cost follows the postings and the pairs that share something -- and suits
 * whole sets (limit == 0 only) of many values of which most pairs share nothing (with counts: bsk_index_build_counted +
 * bsk_index_search_counted).
 * bsk_compare_plan: a short description that names the kernel and its tile shape; figures = {tiles run, rounds summed over the tiles,
 * most rounds of one tile} (a round stages one window of values per set of a tile).
 * bsk_compare_fetch: rows first_row .. first_row + n_rows - 1 to the host, n_rows * n_b cells each; BSK_ERR_ARG for a range outside
 * the matrix, for more cells than cell_cap and for a foreign context. */
int bsk_sets_bottom(bsk_ctx *ctx, const bsk_sets *s, uint64_t n, bsk_sets **out);

typedef struct bsk_compare bsk_compare;
int bsk_sets_compare(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp);
int bsk_compare_info(const bsk_compare *c, uint64_t *n_a, uint64_t *n_b, uint64_t *limit);       /* any out-pointer may be NULL */
int bsk_compare_plan(const bsk_compare *c, const char **plan, uint64_t figures[3]);              /* either may be NULL */
int bsk_compare_fetch(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows,
                      uint32_t *shared, uint32_t *total, uint64_t cell_cap);                      /* either array may be NULL */
int bsk_compare_device(const bsk_compare *c, const uint32_t **shared, const uint32_t **total);
void bsk_compare_release(bsk_compare *c);

/* ---- abundance-weighted all-pairs comparison of counted sets ----
 * bsk_sets_compare_counted walks every pair exactly as bsk_sets_compare does -- the first `limit` distinct values of a[i] | b[j],
 * ascending (limit == 0: all of them) -- so shared and total are, cell for cell, what bsk_sets_compare gives on the same operands and
 * limit.  Over the walked values v that BOTH sets hold, with ca(v) and cb(v) their counts, it also keeps two dense row-major u64
 * matrices on the device:
 *   dot[i * n_b + j]     = sum of ca(v) * cb(v), saturating at 2^64-1 (one product of two u32 always fits, the sum need not; saturating
 *                          addition of non-negative terms is associative, so the cell is min(true sum, 2^64-1) whatever the order);
 *   min_sum[i * n_b + j] = sum of min(ca(v), cb(v)), exact (fewer than 2^32 values of counts below 2^32 cannot overflow).
 * A value that only one of the sets holds contributes to neither.  An uncounted operand counts 1 for every value, as in
 * bsk_sets_op_counted; with both operands uncounted dot == min_sum == shared.  Operand limits (2^32 values together, 2^31 cells,
 * checked before anything is allocated), a == b, empty operands, and the *cmp and error rules are those of bsk_sets_compare.
 * Re-use: *cmp may be the object of either compare.  The object remembers which one wrote it last: a bsk_sets_compare into a weighted
 * object leaves it unweighted and keeps the two arrays (as a counted bsk_sets written by an uncounted entry).
 * bsk_compare_info / _plan / _fetch / _device work unchanged on a weighted result; the plan names the kernel (k_cmp_tile_w) and its
 * window.  bsk_compare_weights_device: both NULL for an unweighted result.  bsk_compare_fetch_weights: row-range, cap and
 * foreign-context rules of bsk_compare_fetch; BSK_ERR_ARG for an unweighted result.
 * What the numbers are for (limit == 0), with bsk_sets_sumsq and bsk_sets_totals of the operands:
 *   cosine            dot / (sqrt(sumsq(a)[i]) * sqrt(sumsq(b)[j]))       (sourmash compare's angular similarity is 1 - 2 acos(cosine) / pi)
 *   sum of max        totals(a)[i] + totals(b)[j] - min_sum               (no third matrix is kept)
 *   weighted Jaccard  min_sum / sum of max;   Bray-Curtis dissimilarity  1 - 2 min_sum / (totals(a)[i] + totals(b)[j])
 * bsk_sets_sumsq: per set of the range the sum of its squared counts (the squared norm of the abundance vector), saturating at 2^64-1;
 * an uncounted object gives the sets' sizes; range rules of bsk_sets_totals. */
int bsk_sets_compare_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit, bsk_compare **cmp);
int bsk_compare_weights_device(const bsk_compare *c, const uint64_t **dot, const uint64_t **min_sum);   /* either may be NULL */
int bsk_compare_fetch_weights(bsk_ctx *ctx, const bsk_compare *c, uint64_t first_row, uint64_t n_rows,
                              uint64_t *dot, uint64_t *min_sum, uint64_t cell_cap);                       /* either array may be NULL */
int bsk_sets_sumsq(bsk_ctx *ctx, const bsk_sets *s, uint64_t first, uint64_t count, uint64_t *sumsq /* host */);

/* ---- weighted containment search: a counted index, dot and min_sum per hit ----
 * The abundance-weighted form of bsk_index_build + bsk_index_search, the route whose cost follows the postings and not the cells: a
 * counted sample (bsk_result_sets_counted) against an index of 10^5 genomes, or a panel of counted samples against itself.
 * Definition.  For a listed pair (q, t) with V = q & t over the whole sets, cq(v) the query's count of v (1 for uncounted queries) and
 * ct(v) the target's (1 for an index without counts):
 *   dot     = min(sum over v in V of cq(v) * ct(v), 2^64-1)     (saturating; exactly this minimum, whatever the order of the adds)
 *   min_sum = sum over v in V of min(cq(v), ct(v))              (exact: fewer than 2^32 values of counts below 2^32)
 * -- the cells of bsk_sets_compare_counted and the weights of bsk_sets_neighbors_counted with limit == 0.  With both operands
 * uncounted dot == min_sum == shared.
 * bsk_index_build_counted is bsk_index_build plus a device array post_cnt[n_postings] (u32) parallel to the posting lists -- the
 * target's count of the value -- and two per-target arrays, sumsq[n_targets] (u64, saturating, as bsk_sets_sumsq) and
 * totals[n_targets] (u64, as bsk_sets_totals).  The index owns copies of everything, so the sets may be released.  Every array of
 * bsk_index_build (keys, posting offsets, target ids, directory, sizes) and bits and max_bucket are bit-identical to bsk_index_build of
 * the same sets; device_bytes grows by the new arrays.  Uncounted targets give an index without counts, exactly what bsk_index_build
 * gives.  Limits, argument checks and *out ("only writes its slot": NULL on every error) are those of bsk_index_build, which itself is
 * unchanged: given counted sets it still builds an index without counts.
 * bsk_index_counted: *counted = 1 iff the index keeps counts.
 * bsk_index_fetch_norms: sumsq and totals of targets first .. first + count - 1 to the host; either out array may be NULL; range and
 * foreign-context rules of bsk_sets_totals.  An index without counts reports |t| for both.
 * bsk_index_search_counted: offsets, target and shared are bit-identical to bsk_index_search with the same arguments -- the thresholds
 * read shared only, the weights are a payload -- and the hits also carry dot[n_hits] and min_sum[n_hits] (bsk_hits_weights_device,
 * bsk_hits_fetch_weights); they carry no totals and no members.  Any of the four combinations of counted and uncounted queries and index
 * is legal.  The argument checks and their order (null, foreign context, reserved, covers), the 2^32 limits and the *hits rules are
 * those of bsk_index_search ("The result slot" above).  After the search a payload pass visits every posting of every query value
 * once more and looks its target up in the query's finished row: queries of the search's small path whose row holds at most 512 hits
 * take a wavefront each and accumulate in LDS (k_sw_row); the others are cut into chunks of 256 query values that spread over the
 * device and add with 64-bit atomics (k_sw_chunk).  Integer adds commute: the result is bit-identical from call to call.
 * bsk_hits_plan gives the search's own text followed by "; weights: k_sw_row ... queries ..., k_sw_chunk ... chunks ..."; its count of
 * large queries is the search's.
 * On a counted index bsk_index_search, the pipeline's hits sink and bsk_index_info work exactly as on a plain one; bsk_index_attach
 * shares the new arrays on the same device and copies them to another device.  Re-use: *hits may be any bsk_hits of this context;
 * every entry that writes hits without weights (bsk_index_search, bsk_hits_top, bsk_hits_fold, the hits sink, ...) leaves the object
 * without weights and keeps the arrays.  Not here: thresholds on the weighted measures, weights that survive bsk_hits_top or
 * bsk_hits_fold, a weighted hits sink in the pipeline.
 * What the numbers are for, with bsk_sets_sumsq / bsk_sets_totals of the queries and bsk_index_fetch_norms of the index: the cosine,
 * the weighted Jaccard and the Bray-Curtis dissimilarity of every hit (formulas: bsk_sets_compare_counted); against an index without
 * counts dot / totals(q) is the share of the query's k-mer mass that falls in the target. */
int bsk_index_build_counted(bsk_ctx *ctx, const bsk_sets *targets, bsk_index **out);
int bsk_index_counted(const bsk_index *ix, int *counted);
int bsk_index_fetch_norms(bsk_ctx *ctx, const bsk_index *ix, uint64_t first, uint64_t count, uint64_t *sumsq, uint64_t *totals); /* either array may be NULL */
int bsk_index_search_counted(bsk_ctx *ctx, const bsk_index *ix, const bsk_sets *queries, const bsk_search_params *sp, bsk_hits **hits);

/* ---- window sets and folded hits: genome chunks as search targets ----
 * kmcp indexes one k-mer set per CHUNK of a reference (--split-number, --split-size, --split-overlap) and counts how many chunks of a
 * genome a read set hits (--min-chunks-fraction); fastANI and skani work on fragments in the same way.  Two entries serve that
 * workflow on the device: genome -> window sets -> index; reads -> search -> hits folded per genome, with the chunks hit -> top.
 *
 * bsk_result_sets_windows: one set per window of a sequence.
 *   Tuple j of a sequence has position p = pos[] & ~BSK_POS_STRAND_BIT.  For the every-position kinds, whose pos is NULL, p = j.
 *   A sequence with c tuples has last position P.
 *   In count mode (wp->count != 0), for that sequence, W = max(1, ceil((P + 1) / count)) and S = W.
 *   In all other cases W = window and S = step ? step : window.
 *   first(p) = p < W ? 0 : (p - W) / S + 1.  With S == W this is p / W.
 *   The sequence has nwin = c ? first(P) + 1 : 0 windows.
 *   Window w holds the tuples with w*S <= p < w*S + W.
 *   Consequences: every tuple lies in at least one window; with S < W a tuple lies in several windows; interior windows without
 *   tuples are empty sets; in count mode nwin <= count.
 *   The window count is derived from the TUPLES, not from the sequence length: a result does not keep lengths.  A sequence whose
 *   last bases select no tuple has fewer windows than its length would give, and a sequence without tuples has none.
 *   Set number seq_offsets[i] + w is window w of sequence i, and seq_offsets[n_reads] equals the number of sets.  seq_offsets is a
 *   host array of n_reads + 1 entries, or NULL.
 *   Values are handled exactly as in bsk_result_sets: distinct and ascending, through the FracMinHash filter hash <= MaxUint64/scale;
 *   with BSK_WINDOWS_COUNTED each value carries its run length inside the window (a counted bsk_sets).
 *   The output is an ordinary bsk_sets: index, search, op, reduce, compare, neighbours and fetch all work unchanged.  By construction
 *   bsk_sets_reduce(windows, seq_offsets, n_reads, 1) equals bsk_result_sets(r, BSK_SETS_PER_SEQUENCE, scale) value for value, for any step.
 *   Errors.  BSK_ERR_ARG, which keeps the slot: a NULL ctx, r, wp or sets; both or neither of window and count set; step > window; step
 *   set in count mode; window >= 2^31; an unknown flag bit; scale < 0; a result or *sets of another context.  BSK_ERR_UNSUPPORTED (2^32
 *   or more windows in total, or 2^32 or more gathered tuples with the overlap multiplicity counted: both totals are known after a
 *   read-back), BSK_ERR_NOMEM and BSK_ERR_DEVICE release the slot.
 *   How it runs.  A sequence's tuples are stored in position order, so a window is a contiguous span (first tuple, count, stride) of
 *   them, found by two searches over the sequence's positions (k_win_count, the library's scan, k_win_spans); the spans -- which may
 *   overlap -- then go through the very path of bsk_result_sets: its small-set kernel, its segmented sort, its filter, its counts.
 *
 * bsk_hits_fold: hits by target group, with the members hit.
 *   Group g is targets group_offsets[g] .. group_offsets[g + 1] - 1; group_offsets[0] == 0, non-decreasing, the last at most 2^32 and
 *   n_groups < 2^32, else BSK_ERR_ARG (checked on the host).  Empty groups are legal.  The pointer is not retained.
 *   The output has the rows of h.  Per row there is one hit for every group of which the row hit at least one target and which passes
 *   both conditions of fp: target = g, ascending inside the row; shared = the sum of the members' shared, saturating at 2^32-1;
 *   members = how many of the group's targets the row hit, a fifth u32 array parallel to target (bsk_hits_members_device,
 *   bsk_hits_fetch_members).  A group is kept iff members >= max(min_members, 1) and, with frac_den != 0,
 *   (uint64_t)members * frac_den >= (uint64_t)frac_num * group_size (exact: no rounding, no division).  fp == NULL is {1, 0, 0, 0}.
 *   members follows the rule of total and the weights: every entry that writes hits without members into a re-used object leaves it
 *   without members; the array is kept and only grows.  The output carries neither totals nor weights, whatever h carried.
 *   bsk_hits_info / _fetch / _top / _cluster / _release work on it unchanged; the output of bsk_hits_top carries no members.
 *   The input must have targets strictly ascending inside every row: search, neighbours and from-host results do, bsk_hits_top results
 *   do not.  One small device pass (k_fold_check) finds a row that is not strictly ascending and a target >= group_offsets[n_groups]
 *   before the object is taken over: both are BSK_ERR_ARG and keep the slot.  So do *out == h, a foreign context, a NULL argument, a
 *   flag bit, frac_num > frac_den with frac_den != 0, and the 2^32 limits (rows, hits: BSK_ERR_UNSUPPORTED).  BSK_ERR_NOMEM and
 *   BSK_ERR_DEVICE release the slot.  n_queries == 0 gives an empty result with BSK_OK.
 *   How it runs: a u32 map target -> group (k_fold_map); a head where a row starts or the group changes (k_fold_check); the library's
 *   scan; every head's owner walks its run and sums it (k_fold_runs); the kept runs are placed (k_fold_place).  No atomics on the
 *   output and no kernel that waits on another: the result is bit-identical from call to call.  bsk_hits_plan names the kernels and
 *   reports groups= and kept= as decimal figures; n_large_queries is 0.
 *   bsk_hits_members_device: *members = NULL for hits without members.  bsk_hits_fetch_members: the members of the hits of rows first ..
 *   first + count - 1, with the range, cap and foreign-context rules of bsk_hits_fetch_totals; BSK_ERR_ARG for hits without members. */
enum { BSK_WINDOWS_COUNTED = 1 };
typedef struct bsk_window_params {
    uint32_t window;  /* positions per window; 0 iff count != 0 */
    uint32_t step;    /* distance between window starts; 0 = window (no overlap); 1 <= step <= window */
    uint32_t count;   /* != 0: `count` windows per sequence, sized per sequence (kmcp --split-number); window and step must be 0 */
    uint32_t flags;   /* BSK_WINDOWS_COUNTED or 0; any other bit: BSK_ERR_ARG */
} bsk_window_params;
int bsk_result_sets_windows(bsk_ctx *ctx, const bsk_result *r, const bsk_window_params *wp, int scale,
                            bsk_sets **sets, uint64_t *seq_offsets /* host, [n_reads + 1], or NULL */);
typedef struct bsk_fold_params {
    uint32_t min_members;  /* keep a group only if >= this many of its targets were hit; 0 is taken as 1 */
    uint32_t flags;        /* 0; any bit: BSK_ERR_ARG */
    uint32_t frac_num;     /* with frac_den != 0: keep iff members * frac_den >= frac_num * group_size (u64, exact) */
    uint32_t frac_den;     /* 0: no such condition; frac_num > frac_den with frac_den != 0: BSK_ERR_ARG */
} bsk_fold_params;
int bsk_hits_fold(bsk_ctx *ctx, const bsk_hits *h, const uint64_t *group_offsets /* host, [n_groups + 1] */, uint64_t n_groups,
                  const bsk_fold_params *fp /* NULL: {1,0,0,0} */, bsk_hits **out);
int bsk_hits_members_device(const bsk_hits *h, const uint32_t **members);  /* NULL for hits without members */
int bsk_hits_fetch_members(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *members, uint64_t hit_cap);

/* ---- hits selected by a measure: an exact filter, a top-n that keeps the payloads ----
 * bsk_hits_filter keeps the hits whose measure reaches a threshold, bsk_hits_top_by keeps every row's n hits of largest measure.  Both
 * carry every payload h carries -- total, dot / min_sum, members -- with the same has-flags, so thresholds on the weighted measures,
 * the k nearest neighbours by cosine, the best genome of a fold with its members and clustering by a weighted measure
 * (filter, then bsk_hits_cluster) all stay on the device.  bsk_hits_top itself is unchanged and still drops the payloads.
 * The measure.  Every measure of hit i is an exact fraction N/D of non-negative integers.  The hit belongs to query q and has target t,
 * Q = qnorm[q] and T = tnorm[t]:
 *   BSK_MEASURE_SHARED            N = shared          D = 1
 *   BSK_MEASURE_MEMBERS           N = members         D = 1                      needs hits with members
 *   BSK_MEASURE_DOT               N = dot             D = 1                      needs weights
 *   BSK_MEASURE_MIN_SUM           N = min_sum         D = 1                      needs weights
 *   BSK_MEASURE_QUERY_COV         N = shared          D = Q                      qnorm: the queries' sizes
 *   BSK_MEASURE_TARGET_COV        N = shared          D = T                      tnorm: the targets' sizes
 *   BSK_MEASURE_JACCARD           N = shared          D = total[i] where h has totals, else Q + T - shared (both norms: sizes)
 *   BSK_MEASURE_COSINE            N = dot * dot       D = Q * T                  weights, both norms: bsk_sets_sumsq
 *   BSK_MEASURE_WEIGHTED_JACCARD  N = min_sum         D = Q + T - min_sum        weights, both norms: bsk_sets_totals
 *   BSK_MEASURE_BC_SIMILARITY     N = 2 * min_sum     D = Q + T                  weights, both norms: bsk_sets_totals
 *   BSK_MEASURE_QUERY_MASS        N = dot             D = Q                      weights, qnorm: bsk_sets_totals
 * COSINE's N/D is the squared cosine -- the order is the cosine's, and the filter squares its bound to match.  BC_SIMILARITY is
 * 1 - Bray-Curtis: "dissimilarity <= x" is "similarity >= 1 - x".  A saturated dot is the number 2^64-1, as everywhere else.  D is
 * formed in more than 64 bits (Q + T overflows a u64); N, D and every product below fit 256 bits (wide_uint.hpp).  Integers only: no
 * division, no rounding, no float.
 * qnorm[n_qnorm] and tnorm[n_tnorm] are host arrays, not retained; NULL / 0 where the kind needs none (given anyway, they are ignored).
 * BSK_ERR_ARG, all of which keep the slot: a NULL ctx, h, m or slot; an unknown kind; a flag bit; a payload or a norm the kind needs
 * that is absent; n_qnorm != n_queries where qnorm is needed; *out == h; hits or *out of another context; and, found by one small device
 * pass (k_sel_check) before the object is taken over, a hit with target >= n_tnorm where tnorm is needed and a hit with D <= 0 (norms
 * inconsistent with the hits).  n_queries >= 2^32 or n_hits >= 2^32 is BSK_ERR_UNSUPPORTED and keeps the slot too; BSK_ERR_NOMEM and
 * BSK_ERR_DEVICE release it.  The input need not have ascending rows: the output of bsk_hits_top / _top_by is legal input.
 * bsk_hits_filter: a hit is kept iff N * min_den >= min_num * D; for COSINE iff N * min_den^2 >= min_num^2 * D, so the bound is on the
 * cosine itself.  min_den == 0 is BSK_ERR_ARG.  Rows keep their order, offsets shrink.  How it runs: the flag pass fused with the check
 * (k_sel_check), the library's scan, the new offsets read from the scan at the old offsets (k_sel_offsets) and one placement pass
 * (k_sel_place).  No atomics on the output and no kernel that waits on another: the result is bit-identical from call to call.
 * bsk_hits_plan names the kernels and reports kept= as a decimal figure; n_large_queries is 0.
 * bsk_hits_top_by: per query the min(n, hits) hits of largest measure.  Hit a is better than hit b iff N_a * D_b > N_b * D_a, ties by
 * ascending target (the targets of a row are distinct for everything the library produces); hits are stored best first, as
 * bsk_hits_top stores them.  n == 0 is BSK_ERR_ARG.  With BSK_MEASURE_SHARED offsets, target and shared are bit-identical to
 * bsk_hits_top(h, n).  How it runs: rows of at most 16 hits are ranked by a group of 16 lanes (k_tb_group); rows of at most 1 024 hits
 * have their hit indices sorted by a wavefront in LDS on the bitonic network, with the comparator (k_tb_lds); longer rows take a
 * workgroup each, which sorts a u32 index array in pooled global memory on the same network, __syncthreads() between the steps
 * (k_tb_global: c log^2 c compares by ONE workgroup -- filter first where rows hold far more than 10^4 hits).  Every kernel gathers all
 * arrays by the sorted indices.  bsk_hits_plan reports the queries per path; n_large_queries is the count of the global path. */
enum { BSK_MEASURE_SHARED = 0, BSK_MEASURE_MEMBERS, BSK_MEASURE_DOT, BSK_MEASURE_MIN_SUM,
       BSK_MEASURE_QUERY_COV, BSK_MEASURE_TARGET_COV, BSK_MEASURE_JACCARD,
       BSK_MEASURE_COSINE, BSK_MEASURE_WEIGHTED_JACCARD, BSK_MEASURE_BC_SIMILARITY, BSK_MEASURE_QUERY_MASS };
typedef struct bsk_measure {
    uint32_t kind, flags;                      /* flags 0; any bit: BSK_ERR_ARG */
    const uint64_t *qnorm; uint64_t n_qnorm;   /* host, not retained; NULL / 0 where the kind needs none */
    const uint64_t *tnorm; uint64_t n_tnorm;
} bsk_measure;
typedef struct bsk_filter_params { uint64_t min_num, min_den; } bsk_filter_params;  /* min_den == 0: BSK_ERR_ARG */
int bsk_hits_filter(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, const bsk_filter_params *fp, bsk_hits **out);
int bsk_hits_top_by(bsk_ctx *ctx, const bsk_hits *h, const bsk_measure *m, uint32_t n, bsk_hits **top);

/* ---- hits by target: the transpose with its payloads, the per-target tally ----
 * Every result of the sets side is a bsk_hits, a CSR by query.  bsk_hits_transpose turns the table round -- which queries hit target t,
 * a target's best query (transpose, then bsk_hits_top_by), reciprocal best hits -- and bsk_hits_tally is the one reduction everybody
 * computes from it: how many hits went to each target and how many of them to that target alone (the table kmcp profile, a Kraken
 * report and mash screen end in).  Neither chooses a policy; both compose with everything that takes hits.
 *
 * bsk_hits_transpose: the output has n_targets rows.  Row t lists, as its target[], the queries q of h that hit t, ascending; should a
 * row of h name t twice (nothing the library produces does), those hits keep their order in h.  shared goes with its hit, and so does
 * every payload h carries -- total, dot / min_sum, members -- with the same has-flags; a re-used *out of any history ends with exactly
 * the flags of h.  Targets nobody hit are empty rows, trailing ones included: n_targets may exceed the largest target + 1.  The input
 * need not have ascending rows: the output of bsk_hits_top / _top_by is legal input.  For an input with ascending rows
 * transpose(transpose(h, n_targets), n_queries) is h, bit for bit, every array included.
 * BSK_ERR_ARG, all of which keep the slot: a NULL ctx, h or out; *out == h; h or *out of another context; and, found by one small
 * device pass (k_tp_keys) before the object is taken over, a hit with target >= n_targets.  n_targets, n_queries or n_hits of 2^32 or
 * more is BSK_ERR_UNSUPPORTED and keeps the slot too; BSK_ERR_NOMEM and BSK_ERR_DEVICE release it.  n_hits == 0, n_queries == 0 and
 * n_targets == 0 (without hits) give empty results with BSK_OK.
 * How it runs: a key (target << hit_bits) | hit index per hit (k_tp_keys), every key distinct; the library's key sort over the
 * key_bits = hit_bits + target_bits that matter; the output offsets by a search of every target's first key (k_tp_offsets); one
 * placement pass that gathers every array by the sorted index and finds the hit's query by a search of h's offsets (k_tp_place).  No
 * atomics on the output, no row of either side walked by one lane, nothing rests on the sort being stable: the result is a function
 * of h and n_targets alone, bit-identical from call to call.  bsk_hits_plan names the kernels and reports targets=, hits= and
 * key_bits= as decimal figures; n_large_queries is 0.
 *
 * bsk_hits_tally: per target t three u64 -- rows[t], the hits of h that name t; unique[t], those among them that are the only hit of
 * their row; shared[t], the sum of their shared.  The sum is exact: 2^32 hits of 2^32 cannot reach 2^64 in one call; across
 * BSK_TALLY_ADD calls the three arrays add modulo 2^64.  Weights, totals and members are not tallied: they are one bsk_hits_transpose
 * away for whoever wants them.
 * Without BSK_TALLY_ADD the table is that of h; a re-used object is overwritten, its arrays are kept and only grow.  With
 * BSK_TALLY_ADD the figures of h are added to those *out holds, and queries, hits and calls of bsk_tally_info add up too; a NULL slot
 * under ADD is a fresh table, a table of another n_targets is BSK_ERR_ARG.
 * BSK_ERR_ARG / BSK_ERR_UNSUPPORTED: those of bsk_hits_transpose, and any other flag bit.  All of them keep the slot, and under ADD
 * the table is unchanged: the target check (k_tl_check) runs, and its answer is read, before anything is added.
 * How it runs: up to 2 048 targets a workgroup of 512 lanes adds into three u64 counters per target in LDS and then adds its non-zero
 * counters to the table, one global add per counter and workgroup (3 x 8 B x 2 048 = 48 KB of a CU's 160 KB: three workgroups, six
 * wavefronts per SIMD); beyond that the adds go straight to the table in global memory.  On both paths a wavefront whose hits all
 * name one target sums on its lanes and adds once.  unique is found per row (offsets difference 1), rows and shared per hit.  The
 * sums are integer adds: bit-identical from call to call.  bsk_tally_plan says which path ran and reports targets= and hits=.
 * bsk_tally_info: n_targets, and the queries, hits and calls the table holds.  bsk_tally_fetch copies targets first .. first + count - 1
 * of the arrays asked for (any pointer may be NULL); first + count > n_targets and a table of another context are BSK_ERR_ARG.
 * bsk_tally_device: the device arrays, n_targets u64 each. */
enum { BSK_TALLY_ADD = 1 };
typedef struct bsk_tally bsk_tally;
int bsk_hits_transpose(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, bsk_hits **out);
int bsk_hits_tally(bsk_ctx *ctx, const bsk_hits *h, uint64_t n_targets, uint32_t flags, bsk_tally **out);
int bsk_tally_info(const bsk_tally *t, uint64_t *n_targets, uint64_t *queries, uint64_t *hits, uint64_t *calls);
int bsk_tally_plan(const bsk_tally *t, const char **plan);
int bsk_tally_fetch(bsk_ctx *ctx, const bsk_tally *t, uint64_t first, uint64_t count,
                    uint64_t *rows, uint64_t *unique, uint64_t *shared);   /* any may be NULL */
int bsk_tally_device(const bsk_tally *t, const uint64_t **rows, const uint64_t **unique, const uint64_t **shared);
void bsk_tally_release(bsk_tally *t);

/* ---- merged hits: one bsk_hits out of the hits of several searches ----
 * An index holds fewer than 2^32 postings and lives on one device; a database beyond that is split into shards, every shard is
 * searched, and bsk_hits_merge joins the results where they are (kmcp merge; sourmash over several databases) -- with every payload,
 * which the route over the host and bsk_hits_from_host drops.  Two ways to shard, one entry: by target (shard p holds the targets
 * target_base[p] .. target_base[p] + T_p - 1: a row of the result is the union of the parts' rows) and by value (every shard holds all
 * targets and a range of the hash space: equal bases, and the integers of a pair that several shards report add up, BSK_MERGE_ADD).
 * It chooses no policy and composes with everything that takes hits.
 *
 * All parts have the same n_queries and the result has those rows.  Row q of the result holds every hit of row q of every part with
 * target' = target + target_base[p] (target_base == NULL: all 0), strictly ascending by target'.  The rows of the parts need not be
 * ascending: the output of bsk_hits_top / _top_by is legal input, so a caller may cut every shard's hits to its n best, merge, and
 * take the n best again.  Two hits of one result row with the same target' -- across parts or inside one part, which nothing the
 * library produces has -- are BSK_ERR_ARG without BSK_MERGE_ADD; with it they become one hit whose fields are the sums, each
 * saturating at its type's maximum: shared, total and members at 2^32 - 1, dot and min_sum at 2^64 - 1.  Saturating sums of
 * non-negative integers do not depend on their order: the result is a function of the inputs alone.  The result carries a payload
 * (total; dot and min_sum; members) if and only if every part carries it; a re-used *out of any history ends with exactly those flags.
 * One part with a base is a relabelling.
 * Parts of ctx are read in place; a part of another context on the same device is read in place after the entry has synchronised
 * that context's stream on the host; a part on another device is copied once into ctx's pool with the peer copy bsk_index_attach
 * uses.  The caller must not write or release a part during the call.  *out is NULL or an object of ctx and not one of the parts.
 * BSK_ERR_ARG, all of which keep the slot, in this order: a NULL ctx, parts or out; n_parts == 0 or > BSK_MERGE_MAX_PARTS; any flag
 * bit but BSK_MERGE_ADD; a NULL parts[p]; rows that differ between parts; *out among the parts; *out of another context; a
 * target_base[p] >= 2^32; and, found on the device before the object is taken over, a duplicate without BSK_MERGE_ADD.
 * BSK_ERR_UNSUPPORTED, which keeps the slot too: 2^32 rows or more, 2^32 hits in total or more, and some target_base[p] + target
 * >= 2^32 (known from the check pass, before the object is taken over).  BSK_ERR_NOMEM and BSK_ERR_DEVICE release it.  n_queries == 0
 * and parts that are all empty give empty results with BSK_OK.
 * How it runs: a small pass per part (k_mg_check, a lane per hit, one ballot per trip of a wavefront) finds the part's smallest and
 * largest target and whether every row is strictly ascending; the host reads one block of figures.  The output offsets before any
 * combining are the sum of the parts' offsets: no scan.  path=concat, when every part has ascending rows and the shifted target
 * ranges of the non-empty parts are disjoint and increase with p (the shards by target): k_mg_starts writes per part and row where
 * the part's hits begin, a lane per row over at most 64 parts whose pointers live in a pool array; k_mg_place, a lane per input hit,
 * finds the hit's row by a search of its part's offsets and writes target + base, shared and every carried payload once.  Every
 * array is read once and written once: no sort, no atomics, no row walked by one lane; duplicates cannot exist here.  path=sort, for
 * everything else: the same placement into pool scratch with the key (target' << idx_bits) | place, every key distinct, so
 * nothing rests on the sort being stable; the library's segmented key sort over the rows; a head where a row starts or target'
 * changes (k_mg_heads); the library's scan over the heads; every head's owner gathers its run by the keys' low bits, sums it and
 * places it (k_mg_runs).  The result is bit-identical from call to call on both paths.  bsk_hits_plan names the kernels and reports
 * path=concat|sort, parts=, hits= (those of the parts in total) and combined= (hits - the result's hits) as decimal figures;
 * n_large_queries is 0. */
enum { BSK_MERGE_ADD = 1 };
enum { BSK_MERGE_MAX_PARTS = 64 };
int bsk_hits_merge(bsk_ctx *ctx, const bsk_hits *const *parts, const uint64_t *target_base /* host, [n_parts], or NULL: all 0 */,
                   uint32_t n_parts, uint32_t flags, bsk_hits **out);

/* ---- clusters of a neighbour graph: connected components and greedy representatives ----
 * (bsk_sets_neighbors, which makes such a graph from sets, is declared below this block: it closes the header.)
 * bsk_hits_cluster turns hits that are already on the device into clusters with one representative each -- n labels and at most n
 * representatives cross the link, whatever the number of edges.
 * The graph of h: the nodes are 0 .. n - 1 with n = n_queries; every hit (i, j) with j != i is an UNDIRECTED edge; diagonal hits and
 * repeated directions are ignored, so the BSK_NEIGHBORS_UPPER result and the full result of one bsk_sets_neighbors(a, a, ...) cluster
 * identically.  shared[] and total[] are not read.  A hit with target >= n (rectangular hits: a != b) is BSK_ERR_ARG.
 * Priority: score[n] (host, not retained) or NULL.  A higher score is a higher priority, ties go to the smaller index; NULL is index
 * order, index 0 best.  rank[v] is v's position in that order, and "best" below means the smallest rank.
 *   BSK_CLUSTER_COMPONENTS  the clusters are the connected components (single linkage at the threshold the hits were made with); the
 *                           representative of a component is its member of best rank.
 *   BSK_CLUSTER_GREEDY      the sequential rule of cd-hit, galah and dRep's second step: visit the nodes by ascending rank; a node that
 *                           neighbours a node which is already a representative joins the one of best rank among those, any other
 *                           node becomes a representative.  Clusters are NOT transitive: a member neighbours its representative,
 *                           members need not neighbour each other.
 * The result, the same layout for both: n_clusters; rep[n_clusters] (u32) ascending by index -- cluster c is the cluster of rep[c];
 * label[n] (u32) the cluster number of every node; offsets[n_clusters + 1] (u64) and members[n] (u32), ascending inside a cluster;
 * the size of the largest cluster.  It is a function of the graph and the scores alone, bit-identical from call to call.
 * cp == NULL is {BSK_CLUSTER_COMPONENTS, 0}; an unknown method or any flag bit is BSK_ERR_ARG.  n >= 2^32 or n_hits >= 2^32 is
 * BSK_ERR_UNSUPPORTED.  n == 0 gives an empty result with BSK_OK.
 * *out follows "The result slot" above: NULL, or a bsk_clusters of this context whose arrays are kept and only grow.  Every
 * BSK_ERR_ARG -- h or *out of another context and a target >= n included, which one small device pass finds before the object is taken
 * over -- and the 2^32 limits keep the slot; BSK_ERR_NOMEM and BSK_ERR_DEVICE release it.
 * How it runs.  Both methods work in rounds that the HOST drives: a round is two small launches over the edges and the nodes, and the
 * host reads one word back to decide whether to go on.  Inside a launch workgroups meet only in 32-bit atomics (min / or / add) whose
 * results nothing reads before the launch ends; everything a kernel reads was written by an earlier launch.  No kernel spins, retries
 * or waits for another workgroup, and the rounds are capped at n + 1, so a defect ends in BSK_ERR_DEVICE, never in a hang -- and the
 * number of rounds is itself a function of the input.  Components hook every edge's larger root under the smaller and halve the paths
 * (k_cl_hook + k_cl_jump): a path of 4 096 nodes takes 14 to 18 rounds, not 4 096.  Greedy decides per round every node whose better
 * neighbours are all decided (k_cl_mis_scan + k_cl_mis_apply): a handful of rounds on graphs in no particular order, but n ROUNDS in
 * the worst case -- a path whose nodes are ranked from one end to the other -- each of them two launches; eight rounds go out per
 * read-back.
 * bsk_clusters_plan: "k_cl_hook+k_cl_jump, n=... edges=... rounds=..." or "k_cl_mis, n=... edges=... rounds=..." with decimal figures,
 * and figures[0] = the rounds (components: the last, unchanged one included; greedy: the last round that decided a node), figures[1] =
 * the hits with j != i.  bsk_clusters_fetch copies the arrays asked for (any pointer may be NULL) into label[n], rep[n_clusters],
 * offsets[n_clusters + 1], members[n]; clusters of another context are BSK_ERR_ARG.  bsk_clusters_device: the device arrays.
 * bsk_hits_from_host, the counterpart of bsk_sets_from_host: hits made elsewhere (ANI, alignments) as CSR -- offsets[n_queries + 1]
 * with offsets[0] == 0 and non-decreasing, target[] strictly ascending inside a row (checked on the host: BSK_ERR_ARG), shared[], and
 * total[] or NULL for hits without totals.  Host pointers are not retained.  *hits follows "The result slot": every BSK_ERR_ARG keeps it,
 * BSK_ERR_NOMEM and BSK_ERR_DEVICE release it.  bsk_hits_plan reports "from host". */
enum { BSK_CLUSTER_COMPONENTS = 0, BSK_CLUSTER_GREEDY = 1 };
typedef struct bsk_cluster_params {
    uint32_t method;   /* BSK_CLUSTER_COMPONENTS or BSK_CLUSTER_GREEDY; anything else: BSK_ERR_ARG */
    uint32_t flags;    /* 0; any bit: BSK_ERR_ARG */
} bsk_cluster_params;
typedef struct bsk_clusters bsk_clusters;
int bsk_hits_cluster(bsk_ctx *ctx, const bsk_hits *h, const bsk_cluster_params *cp /* NULL: {0,0} */,
                     const uint64_t *score /* host, [n_queries], or NULL */, bsk_clusters **out);
int bsk_clusters_info(const bsk_clusters *c, uint64_t *n_items, uint64_t *n_clusters, uint64_t *largest);
int bsk_clusters_plan(const bsk_clusters *c, const char **plan, uint64_t figures[2] /* rounds, edges */);
int bsk_clusters_fetch(bsk_ctx *ctx, const bsk_clusters *c, uint32_t *label, uint32_t *rep, uint64_t *offsets, uint32_t *members); /* any may be NULL */
int bsk_clusters_device(const bsk_clusters *c, const uint32_t **label, const uint32_t **rep, const uint64_t **offsets, const uint32_t **members);
void bsk_clusters_release(bsk_clusters *c);
int bsk_hits_from_host(bsk_ctx *ctx, const uint64_t *offsets, uint64_t n_queries, const uint32_t *target, const uint32_t *shared,
                       const uint32_t *total /* NULL: hits without totals */, bsk_hits **hits);

/* ---- weighted sparse all-pairs comparison: dot and min_sum per kept neighbour ----
 * (bsk_neighbor_params and BSK_NEIGHBORS_UPPER are defined in the block below, which closes the header; nothing here adds a flag or a struct.)
 * bsk_sets_neighbors_counted is bsk_sets_neighbors with the counts of bsk_sets_compare_counted.  The walk, the rule and the result layout
 * are exactly those of bsk_sets_neighbors: offsets, target, shared and total are bit-identical to what bsk_sets_neighbors gives for the
 * same operands, limit and params.  Weights are a payload; they do not take part in the rule -- no threshold reads them.
 * The hits also carry two u64 device arrays parallel to target[]: dot[n_hits] and min_sum[n_hits], defined exactly as the cells of
 * bsk_sets_compare_counted -- over the walked values that both sets hold, dot is the saturating sum of the count products (capped at
 * 2^64-1) and min_sum the exact sum of the minima.  An uncounted operand counts 1 per value; with both operands uncounted
 * dot == min_sum == shared.  With the norms of the operands (bsk_sets_sumsq, bsk_sets_totals) they give the cosine, the weighted Jaccard
 * and the Bray-Curtis dissimilarity of every kept pair (formulas: bsk_sets_compare_counted), without a matrix.
 * The limits (2^32 values together, 2^32 sets each, 2^32 kept pairs, NO limit on cells), a == b and BSK_NEIGHBORS_UPPER -- tiles below
 * the diagonal are never run --, empty operands, the *hits rules ("The result slot" above) and the order of the argument checks (null,
 * flag, fraction, foreign context) are those of bsk_sets_neighbors.
 * Re-use: *hits may be any bsk_hits of this context.  The object remembers whether its last writer kept weights: bsk_index_search,
 * bsk_hits_top, the pipeline's hits sink, bsk_hits_from_host and the unweighted bsk_sets_neighbors leave it without weights and keep the
 * two arrays, which only grow.  bsk_hits_info / _fetch / _totals_device / _fetch_totals / _top / _cluster / _release work unchanged on
 * weighted hits; the output of bsk_hits_top carries neither totals nor weights.
 * bsk_hits_weights_device: both NULL for hits without weights.  bsk_hits_fetch_weights: the weights of the hits of rows first ..
 * first + count - 1, with the range, cap and foreign-context rules of bsk_hits_fetch_totals; BSK_ERR_ARG for hits without weights.
 * bsk_hits_plan names the kernel (k_cmp_tile_nb_w) and carries the same tiles=, skipped=, rounds= and runs= figures; a kept pair takes
 * 32 bytes of the record buffer instead of 16.  The result is bit-identical from call to call. */
struct bsk_neighbor_params;   /* defined in the block below */
int bsk_sets_neighbors_counted(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit,
                               const struct bsk_neighbor_params *np /* NULL: {1,0,0,0} */, bsk_hits **hits);
int bsk_hits_weights_device(const bsk_hits *h, const uint64_t **dot, const uint64_t **min_sum);   /* either may be NULL; both NULL for hits without weights */
int bsk_hits_fetch_weights(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count,
                           uint64_t *dot, uint64_t *min_sum, uint64_t hit_cap);                     /* either array may be NULL */

/* ---- sparse all-pairs comparison: the neighbours above a threshold, no matrix ----
 * bsk_sets_neighbors walks every pair (i, j), i < n_a, j < n_b, exactly as bsk_sets_compare does -- the first `limit` distinct values of
 * a[i] | b[j], ascending (limit == 0: all of them; any u64 is a legal limit) -- so shared and total of a pair are what bsk_sets_compare
 * puts in cell (i, j).  No cell is stored.  The pair is listed iff all three hold:
 *   shared >= max(min_shared, 1)
 *   jaccard_den == 0  ||  (uint64_t)shared * jaccard_den >= (uint64_t)jaccard_num * total       (exact: no rounding, no division)
 *   !(flags & BSK_NEIGHBORS_UPPER)  ||  j > i
 * A pair that shares nothing is never listed, as in the search.  np == NULL is {1, 0, 0, 0}.  A flag bit other than
 * BSK_NEIGHBORS_UPPER, and jaccard_num > jaccard_den with jaccard_den != 0, are BSK_ERR_ARG.
 * The result is an ordinary bsk_hits, CSR by the sets of a: offsets[n_a + 1], target[] = j ascending inside a row, shared[], and a fourth
 * device array total[n_hits] parallel to them (bsk_hits_totals_device, bsk_hits_fetch_totals).  bsk_hits_info / _fetch / _device /
 * _release and bsk_hits_top work on it unchanged -- bsk_hits_top gives the k nearest neighbours of every set; its OUTPUT carries no
 * totals (for bottom-n sketches of full size total == limit anyway).  An entry that writes hits without totals into a re-used object
 * (bsk_index_search, bsk_hits_top, the pipeline's hits sink) leaves it without totals; the array is kept and only grows, like the counts
 * of a counted bsk_sets.  The result is bit-identical from call to call: nothing in it depends on the order in which workgroups finish.
 * BSK_NEIGHBORS_UPPER is defined by the indices, so it is legal for a != b too; with a == b (legal with or without the flag) it lists
 * every unordered pair once, without the diagonal, and the tiles below the diagonal are never run: T (T + 1) / 2 of T x T tiles.
 * Limits: the operands together hold fewer than 2^32 values (a == b: counted once) and each fewer than 2^32 sets (targets are u32), and
 * the call keeps fewer than 2^32 pairs, else BSK_ERR_UNSUPPORTED.  There is NO limit on cells: tiles are counted in 64 bits and memory
 * follows n_a, n_b and the kept pairs, never n_a * n_b.  n_a == 0 or n_b == 0 gives an empty result with BSK_OK.
 * *hits: NULL, or a bsk_hits of this context, wherever it came from ("The result slot" above): an argument error -- hits of another
 * context included -- leaves it as it was, any other error releases it and sets *hits to NULL.
 * Kept pairs are collected in a buffer of records; when a call keeps more than the buffer holds (2^20 the first time, or what a
 * re-used object already holds) the host reads the exact count and the kernel runs once more.  bsk_hits_plan names the kernel
 * (k_cmp_tile_nb) and carries tiles=, skipped=, rounds= and runs= as decimal figures; n_large_queries is 0.
 * bsk_hits_totals_device: *total = NULL for hits without totals.  bsk_hits_fetch_totals: the totals of the hits of rows first ..
 * first + count - 1, with the range, cap and foreign-context rules of bsk_hits_fetch; BSK_ERR_ARG for hits without totals.
 * Which route for an all-against-all: bsk_sets_compare when every cell is wanted and there are at most 2^31 of them;
 * bsk_sets_neighbors when only the pairs above a threshold are (dereplication, clustering, nearest references, the k nearest
 * neighbours), limit-bounded (Mash) numbers included, at any number of cells -- its cost is still the cells (half of them with
 * BSK_NEIGHBORS_UPPER) times the values a pair walks; bsk_sets_neighbors_counted (declared above this block) is the same route
 * with dot and min_sum of every kept pair, for abundance-weighted measures beyond the dense compare's 2^31 cells;
 * bsk_index_build + bsk_index_search for whole sets (limit == 0 only) of many values of which most pairs share nothing -- its
 * cost follows the postings. */
enum { BSK_NEIGHBORS_UPPER = 1 };            /* list only pairs with j > i */
typedef struct bsk_neighbor_params {
    uint32_t min_shared;    /* 0 is taken as 1 */
    uint32_t flags;         /* BSK_NEIGHBORS_UPPER or 0; any other bit: BSK_ERR_ARG */
    uint32_t jaccard_num;   /* with jaccard_den != 0: keep iff shared * den >= num * total (u64, exact) */
    uint32_t jaccard_den;   /* 0: no such condition; num > den with den != 0: BSK_ERR_ARG */
} bsk_neighbor_params;
int bsk_sets_neighbors(bsk_ctx *ctx, const bsk_sets *a, const bsk_sets *b, uint64_t limit,
                       const bsk_neighbor_params *np /* NULL: {1,0,0,0} */, bsk_hits **hits);
int bsk_hits_totals_device(const bsk_hits *h, const uint32_t **total);   /* *total = NULL for hits without totals */
int bsk_hits_fetch_totals(bsk_ctx *ctx, const bsk_hits *h, uint64_t first, uint64_t count, uint32_t *total, uint64_t hit_cap);

#ifdef __cplusplus
}
#endif
#endif /* BIOSKETCH_H */
