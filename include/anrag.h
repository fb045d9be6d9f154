/*
 * anrag.h -- C ABI of libanrag.so: the MI355X (gfx950) retrieval hot path of
 * A-NICE-RAG (dense dot-product top-k, BM25 term-at-a-time top-k, weighted
 * reciprocal-rank fusion) behind plain pointers and sizes.
 *
 * The reference has no FFI of its own: its boundary is the Python method surface
 * of `SearchEngine` (src/search_engine.py:14-293) and `DatabaseManager`
 * (src/database_manager.py:14-99).  Each entry point below names the reference
 * lines it replaces; the Python binding a maintainer would add is shown in
 * INTEGRATION.md and shipped in a-nice-rag_amd/_native.py.
 *
 * Conventions
 *   - every function returns ANRAG_OK (0) or a negative ANRAG_ERR_*; the message
 *     of the last failure on the calling thread is anrag_last_error().  Nothing
 *     throws or aborts across this boundary (the reference's own convention is
 *     "log and return empty", search_engine.py:94-98, :267-269 -- the Python
 *     shim maps error codes back to that).
 *   - "host" pointers are ordinary process memory; "device" pointers are HBM
 *     addresses of the index's GPU (hipMalloc / torch tensor .data_ptr()).
 *     The *_device entry points enqueue on the index's streams and return: a
 *     device INPUT must be complete before the call, and so must any pending
 *     write of the caller's to a device OUTPUT (a framework's zero fill of a
 *     fresh tensor runs on the framework's stream and can land after the answer):
 *     synchronise the producing stream first, or hand the index your streams
 *     (anrag_index_set_streams).
 *   - one anrag_index = one GPU's shard: a row block of the corpus matrix and
 *     the postings of the same documents.  Calls on one index are serialised by
 *     an internal mutex (the reference shares one SearchEngine between Streamlit
 *     session threads, src/app.py:17-27); different indexes are independent.
 *   - document identity inside the library is an int64 "doc id" chosen by the
 *     caller (a global id space shared by the dense rows and the BM25 rows, so
 *     that fusion can run on ids as the reference fuses on chunk-id strings,
 *     search_engine.py:27-32).  Strings never cross the boundary.
 *   - a NaN dense score (a corrupt row, a NaN in the query) ranks FIRST, as numpy's
 *     argpartition / argsort rank it (search_engine.py:83-87); it is reported as
 *     +inf.  BM25 scores cannot be NaN: anrag_bm25_load rejects non-finite idf / avgdl.
 *   - ordering rule everywhere: score descending, then ROW ascending (rows are
 *     what the reference's tie behaviour is stated in: its filtered BM25 path is
 *     a stable sort = low row first, :233; its numpy paths leave ties
 *     unspecified).  Across the ranks of the torch.distributed path the tie-break
 *     is doc id ascending, which is the same thing under row sharding with
 *     doc id = doc_id_base + row; a shard group (below) merges in shard order,
 *     which is (score desc, global row asc) for any doc id map.
 */
#ifndef ANRAG_H
#define ANRAG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANRAG_ABI_VERSION 1

#define ANRAG_OK 0
#define ANRAG_ERR_INVALID (-1) /* bad argument                                   */
#define ANRAG_ERR_HIP (-2)     /* a HIP runtime call failed                      */
#define ANRAG_ERR_STATE (-3)   /* e.g. search before load                        */
#define ANRAG_ERR_NOMEM (-4)   /* host or device allocation failed               */
#define ANRAG_ERR_NODEVICE (-5) /* no usable gfx950 device                       */
#define ANRAG_ERR_UNSUPPORTED (-6) /* the route exists for one index, not for a shard group; or not for this dimension */

/* Largest k served by the fused in-register per-wave top-k (one candidate per
 * lane of a 64-wide wavefront).  Larger k (retrieval_eval.py:142-143 uses 12000)
 * takes the score-array + radix-sort path; both are exact. */
#define ANRAG_FUSED_K_MAX 64
/* Most ranked lists one fusion call takes (the reference fuses at most 4 dense models + BM25). */
#define ANRAG_WRRF_MAX_LISTS 16

/* Candidate record exchanged between shards (RCCL all-gather payload) and
 * consumed by anrag_merge_candidates_device: 16 bytes, score widened to fp64
 * (exact for the dense fp32 scores). Unused slots: doc = -1, score = -inf. */
typedef struct anrag_candidate {
    double score;
    int64_t doc;
} anrag_candidate;

typedef struct anrag_index anrag_index;

/* Kernel ids for anrag_profile_read.
 * With the dense prefilter on, ANRAG_KERNEL_DENSE_SCAN brackets what the route launches on the scan's stream: in the
 * three-stream hybrid pipeline the shadow scan ALONE (threshold and rescore run on the tail's stream, and a bracket
 * cannot span streams); on the one-stream routes (the scan lanes) the shadow scan, the threshold and the rescore. */
#define ANRAG_KERNEL_DENSE_SCAN 0    /* K1: N x D fp32 scan + per-wave top-k      */
#define ANRAG_KERNEL_DENSE_BATCHED 1 /* K2: Q x N fp32 MFMA GEMM + top-k epilogue */
#define ANRAG_KERNEL_BM25 2          /* K3: CSR postings scorer                   */
#define ANRAG_KERNEL_SELECT 3        /* K4: candidate merge / score-array select  */
#define ANRAG_KERNEL_WRRF 4          /* K5: weighted RRF + top-n                  */
#define ANRAG_KERNEL_COUNT 5

/* ------------------------------------------------------------------ library */
int anrag_abi_version(void);
const char *anrag_last_error(void);
int anrag_device_count(int *out_count);

/* ------------------------------------------------------------------ index lifetime
 * Replaces the process-lifetime DataFrame / pickle caches of DatabaseManager
 * (database_manager.py:17-18, :65-66, :92-93): the index owns the HBM copies. */
int anrag_index_create(int device, anrag_index **out);
int anrag_index_destroy(anrag_index *idx);
/* Run the index's kernels on caller-owned HIP streams (hipStream_t as void*).
 * NULL = the index's own streams.  Roles:
 *   primary    dense scans (and every non-hybrid entry point)
 *   secondary  the BM25 leg of a hybrid query and, behind it, the fusion kernel
 *              of anrag_hybrid_search_device (its results are complete in
 *              secondary-stream order; anrag_index_sync waits for everything)
 *   fusion     anrag_merge_candidates_device, anrag_wrrf_device and the
 *              copy-out of anrag_hybrid_candidates_device.  Pass the stream a
 *              torch.distributed (RCCL) collective will be issued on, e.g. a
 *              torch.cuda.Stream's .cuda_stream, and the collective orders
 *              after the per-shard candidates with no host sync. */
int anrag_index_set_streams(anrag_index *idx, void *primary, void *secondary, void *fusion);
/* Block until everything enqueued on the index's streams has finished. */
int anrag_index_sync(anrag_index *idx);
/* Stream ordering WITHOUT a host sync, for callers that keep their own streams (a framework's current stream):
 *   anrag_index_wait_stream    everything the index enqueues from now on runs after the work ALREADY enqueued on
 *                              `stream` (hipStream_t as void*, NULL = the null stream): call it after producing
 *                              device inputs AND after allocating / filling device outputs on that stream (a
 *                              framework's zero fill of a fresh tensor would otherwise race the library's answer),
 *                              before the *_device call;
 *   anrag_index_signal_stream  everything enqueued on `stream` from now on runs after the work already enqueued
 *                              on the index's three streams: call it after the *_device call(s), before the
 *                              framework reads the results on its stream.
 * The default recipe of INTEGRATION.md ("Streams"); anrag_index_set_streams is the alternative that removes the
 * index's own streams altogether. */
int anrag_index_wait_stream(anrag_index *idx, void *stream);
int anrag_index_signal_stream(anrag_index *idx, void *stream);

/* ------------------------------------------------------------------ dense: load
 * The upload point that replaces per-row np.frombuffer + DataFrame
 * (database_manager.py:39-66) and the per-query np.stack (search_engine.py:80):
 * `embeddings` is the row-major n_rows x dim fp32 matrix (host or device
 * pointer), copied once into HBM.  A device operand must be complete when the
 * call is made (synchronise the stream that produced it): the copy runs on the
 * index's own stream and the call returns when it has finished.
 *   source_id  nullable, n_rows x uint16: interned `source` string of each row
 *              (the column the filter of search_engine.py:36-55 looks at)
 *   doc_id     nullable, n_rows x int64: global doc id of each row; NULL means
 *              doc id = doc_id_base + row */
int anrag_dense_load(anrag_index *idx, const float *embeddings, int64_t n_rows, int32_t dim,
                     const uint16_t *source_id, const int64_t *doc_id, int64_t doc_id_base);

/* ------------------------------------------------------------------ dense: search
 * SearchEngine.similarity_search_with_embedding, search_engine.py:57-98 (and the
 * arithmetic of similarity_search, :100-146): raw dot product of each query with
 * every allowed row, top-k by (score desc, row asc).
 *   queries       host, n_queries x dim fp32 (the reference is batch=1,
 *                 search_engine.py:77-81; n_queries > 1 = that loop, batched)
 *   allow_source  nullable host, n_sources bytes: allow_source[s] != 0 keeps rows
 *                 whose source_id == s (the Python shim evaluates the reference's
 *                 prefix/regex rule once per distinct source string)
 *   out_doc / out_score   host, n_queries x k, rank order; unused tail: -1 / -inf
 *   out_count     host, n_queries: entries returned (min(k, allowed rows)) */
int anrag_dense_search(anrag_index *idx, const float *queries, int32_t n_queries, int32_t k,
                       const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc,
                       float *out_score, int32_t *out_count);

/* The same for ONE fp64 query: the reference's text path gets float64 from the
 * embedding API and np.dot then promotes the fp32 matrix and scores in fp64
 * (search_engine.py:157, :129).  Rows stay fp32 in HBM; every dot product is
 * accumulated in fp64 (fp32 values are exact in fp64), selection by sorting the
 * fp64 score array: any k.  out_score: fp64.  (The fp32 entry points round an
 * fp64 query to fp32 first -- inside the 1e-4 bar, not the reference's bits;
 * the Python shim calls this one when it is handed a float64 query.)
 * k <= ANRAG_FUSED_K_MAX and dim % 4 == 0, dim <= 3072: a streaming scan that keeps per-wave fp64 lists (K1D) and
 * the list merge answer instead -- no score array, no sort; the same ids and the same score BITS (one summation order
 * in both kernels).  Its list buffer (512 KB) is allocated by the first such query.
 * While a form of the dense prefilter is built (anrag_set_dense_prefilter) and the list scan serves, the query goes
 * through the shadow prefilter instead of K1D (anrag_set_dense_f64_prefilter): the shadow scan and the threshold kernel
 * run with the query rounded to fp32, the rows whose upper bound reaches the threshold less twice a per-query widening
 * w are rescored with K1D's arithmetic, and the same list merge answers -- the same ids and score bits again, from a
 * quarter (int8) or half (fp16) of the bytes.  The first such query after a dense load also computes the corpus's
 * largest row norm (one extra kernel and host wait). */
int anrag_dense_search_f64(anrag_index *idx, const double *query, int32_t k,
                           const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc,
                           double *out_score, int32_t *out_count);

/* Route of anrag_dense_search_f64 (search_engine.py:157, :129): 1 (default) the list scan wherever it serves, 0 the
 * score array + sort for every k (A/B measurements, the tests that hold the two routes to the same bits).  The
 * answers do not depend on it, except that a score of exactly -0.0 ties with +0.0 by row in the list scan and ranks
 * behind it in the sort. */
int anrag_set_dense_f64_scan(anrag_index *idx, int32_t on);

/* Cumulative fp64 queries answered by the list scan (anrag_hybrid_search_f64's dense legs included) and by the score
 * array + sort.  `scanned` counts every fp64 query answered from per-wave lists: K1D's and the shadow prefilter's. */
int anrag_dense_f64_stats(anrag_index *idx, int64_t *scanned, int64_t *sorted);

/* Route of the fp64 dense leg (anrag_dense_search_f64 with k <= ANRAG_FUSED_K_MAX, anrag_hybrid_search_f64) while a
 * prefilter form is built and the list scan is on and serves the dimension: 1 (default) the shadow prefilter with
 * K1D's rescoring, 0 K1D.  Without a built form it has no effect.  The answers never depend on it.  The environment
 * variable ANRAG_DENSE_F64_PREFILTER=0|1, read at anrag_index_create, sets the initial value. */
int anrag_set_dense_f64_prefilter(anrag_index *idx, int32_t on);

/* Cumulative counters of the fp64 prefilter route since the first such query after the last anrag_dense_load: queries
 * it answered and rows it rescored (waits for the index's streams).  Separate from anrag_dense_prefilter_stats, which
 * counts fp32 queries only. */
int anrag_dense_f64_prefilter_stats(anrag_index *idx, int64_t *queries, int64_t *survivors);

/* Same, all operands in HBM, no host sync: d_out is n_queries x k anrag_candidate.
 * n_queries > 1: up to 8 queries share a scan launch (each is still its own pass over the matrix; a workgroup starts
 * the next query when it has finished this one); every query's list merge runs on the fusion stream under the following
 * scans: results are complete in fusion-stream order.
 * n_queries == 1 on the index's own streams (no anrag_index_set_streams): consecutive calls rotate over up to 4 scan
 * streams whose kernels overlap, and a query's list merge rides in the NEXT scan launch of its stream -- no marker, no
 * merge launch per query (a launch boundary, ramp and drain are a fifth of a 100k-row pass).  Results are complete
 * after anrag_index_sync or behind anrag_index_signal_stream (which launch the merges still pending).
 * d_allow_bits: nullable device bitmap, bit s of word s/32 = source s allowed. */
int anrag_dense_search_device(anrag_index *idx, const float *d_queries, int32_t n_queries,
                              int32_t k, const uint32_t *d_allow_bits, anrag_candidate *d_out);

/* K2: up to 256 queries in ONE pass over the corpus on the fp32 matrix cores
 * (v_mfma_f32_32x32x2_f32: exact f32 products and sums, no bf16 rounding), exact
 * top-k through a sampled-threshold filter (dense_batched.hip).  All operands in
 * HBM, primary stream, no host sync.  d_flag[q] = 0, or -1 when query q's
 * survivor list overflowed and the caller must redo it with
 * anrag_dense_search_device (anrag_dense_search does this by itself and picks
 * this path on its own for n_queries >= 16 on corpora of >= 65536 rows). */
int anrag_dense_search_batch_device(anrag_index *idx, const float *d_queries, int32_t n_queries,
                                    int32_t k, const uint32_t *d_allow_bits, anrag_candidate *d_out,
                                    int32_t *d_flag);

/* Arithmetic of the batched path.  0 (default): exact f32 products and sums on the f32 matrix cores.
 * 1: split-precision -- every operand as hi + lo bf16, three bf16 MFMAs per product (hi.hi + hi.lo + lo.hi),
 * f32 accumulation: scores within ~3e-5 of the f32 result for unit-norm vectors (inside the 1e-4 bar, not
 * bit-equal), ~2.7x the throughput of mode 0.  Applies to passes of any size (the query block is padded to
 * 256).  MEMORY: the first mode-1 pass after a dense load builds a second copy of the corpus as bf16 hi / lo
 * images (4 bytes per element, i.e. the corpus size again; counted in anrag_index_stats' hbm_bytes); it is
 * dropped by the next anrag_dense_load / anrag_index_destroy, not by switching back to mode 0. */
int anrag_set_batched_precision(anrag_index *idx, int32_t mode);

/* Route of the dense top-k leg (k <= ANRAG_FUSED_K_MAX, every entry point that keeps lists: single, grouped, hybrid,
 * sharded).  The results do not depend on it: ids and fp32 scores are bit-identical in every mode.
 * 0: the fp32 scan.  1: the fp16 prefilter -- an fp16 copy of the corpus is scanned, rows that provably cannot reach
 * the top k are dropped, and the few left are rescored with the fp32 scan's own arithmetic (half the bytes per query).
 * 2: the int8 prefilter -- the same with an int8 copy and one scale per row (a quarter of the bytes per query).
 * -1 (default): the int8 prefilter when the fp32 corpus is larger than 1 GiB and the dimension has a kernel shape (a
 * multiple of 256 up to 2,048); when it cannot allocate it silently stays on the fp32 scan, where modes 1 and 2 return
 * ANRAG_ERR_NOMEM.
 * MEMORY: mode 1 n_rows * (2 * dim + 4) bytes for the fp16 copy and the per-row error radii; mode 2 n_rows * (dim + 16)
 * bytes for the int8 copy and the per-row scale and radii; either plus 4 * n_rows bytes per pipeline slot (32) for the
 * rows' score bounds.  One form is held at a time (switching between 1 and 2 replaces it); counted in
 * anrag_index_info's hbm_bytes, built by the first load or call that turns it on, dropped by the next
 * anrag_dense_load / anrag_index_destroy (not by switching to mode 0).
 * The environment variable ANRAG_DENSE_PREFILTER=0|1|2, read at anrag_index_create, sets the initial mode. */
int anrag_set_dense_prefilter(anrag_index *idx, int32_t mode);

/* Cumulative counters of the prefilter since its current form was built: queries it answered and rows it rescored
 * (waits for the index's streams). */
int anrag_dense_prefilter_stats(anrag_index *idx, int64_t *queries, int64_t *survivors);

/* The int8 prefilter's pair pass: two queued queries share one walk of the shadow image (half the bytes per query; every
 * value written per query is the single pass's, bit for bit).  Groups of queries (anrag_hybrid_candidates_group_device,
 * anrag_dense_search_device with n_queries > 1, the per-query branch of anrag_hybrid_search_batch, shard groups) take it
 * two at a time, an odd last query a single pass.  mode: 0 off (single passes only, nothing is ever held), 1 (default)
 * on, and single anrag_hybrid_search_device calls pair by the launch rule given there, 2 as 1 but a lone
 * anrag_hybrid_search_device query is ALWAYS held until a partner or a flushing call arrives (deterministic: for tests).
 * The answers never depend on it.  The environment variable ANRAG_SCAN_PAIR=0|1|2, read at anrag_index_create, sets the
 * initial mode. */
int anrag_set_scan_pairing(anrag_index *idx, int32_t mode);

/* Cumulative int8 scan passes over the image by form -- a pair pass serves two queries, a single pass one -- and whether
 * a query is held at this moment (1 or 0).  Reads without launching the held query and without waiting; NULL outputs are
 * skipped. */
int anrag_scan_pair_stats(anrag_index *idx, int64_t *pair_passes, int64_t *single_passes, int32_t *pending);

/* All N scores of one query (what search_engine.py:81 materialises), for tests
 * and for callers that post-process scores themselves.  out: host, n_rows fp32. */
int anrag_dense_scores(anrag_index *idx, const float *query, float *out_scores);

/* ------------------------------------------------------------------ BM25: load
 * Replaces the pickled rank_bm25.BM25Okapi object (database_manager.py:77-99;
 * built at processing/bm25_search.py:77): term-major CSR postings plus the
 * statistics BM25Okapi.__init__ derives.  All host pointers.
 *   indptr    n_terms+1 offsets into post_doc/post_tf; documents strictly
 *             ascending inside each term
 *   post_doc  document ROW (0..n_docs-1) of each posting;  post_tf  term frequency
 *   idf       n_terms, already epsilon-floored (Python floats from math.log)
 *   doc_len   n_docs token counts;  avgdl, k1, b as BM25Okapi holds them
 *   source_id / doc_id / doc_id_base   as for anrag_dense_load (BM25 rows are a
 *             different row space from the dense rows: bm25_search.py:67-68) */
int anrag_bm25_load(anrag_index *idx, const int64_t *indptr, int64_t n_terms,
                    const int32_t *post_doc, const int32_t *post_tf, const double *idf,
                    const int32_t *doc_len, int64_t n_docs, double avgdl, double k1, double b,
                    const uint16_t *source_id, const int64_t *doc_id, int64_t doc_id_base);

/* ------------------------------------------------------------------ BM25: search
 * SearchEngine._core_bm25_search, search_engine.py:205-243, including the
 * bm25.get_scores call at :219 (rank_bm25 arithmetic: fp64, term-at-a-time in
 * query order, duplicates counted again).  term_ids: host, query tokens mapped
 * to term ids IN QUERY ORDER; a negative id = token not in the vocabulary
 * (contributes nothing).  Zero-score documents are ranked, not dropped.
 * Bit-exact fp64 scores; order (score desc, row asc). */
int anrag_bm25_search(anrag_index *idx, const int32_t *term_ids, int32_t n_terms, int32_t k,
                      const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc,
                      double *out_score, int32_t *out_count);
/* Same, operands in HBM, no host sync: the BM25-only member of the query pipeline (it
 * takes a pipeline slot like anrag_hybrid_search_device does, so it may be mixed
 * freely with hybrid and dense queries in flight).  K3 runs on the secondary
 * stream, the list merge on the fusion stream: d_out (k records) is complete in
 * fusion-stream order (anrag_index_sync waits for everything).  n_terms == 0
 * ranks the all-zero score array, as anrag_bm25_search does. */
int anrag_bm25_search_device(anrag_index *idx, const int32_t *d_term_ids, int32_t n_terms,
                             int32_t k, const uint32_t *d_allow_bits, anrag_candidate *d_out);
/* The same for n_queries queries in one call: d_term_ids / d_out are HOST arrays of device pointers, n_terms a host
 * array.  The queries run in groups of 16 per K3 launch (every query its own workgroups; launch, ramp and drain are paid
 * once per group: 6.5 us per query in the kernel at 1M documents against 7.8 at 8 per launch and 13.5 alone); each takes a
 * pipeline slot like a single call. */
int anrag_bm25_search_group_device(anrag_index *idx, const int32_t *const *d_term_ids, const int32_t *n_terms,
                                   int32_t n_queries, int32_t k, const uint32_t *d_allow_bits,
                                   anrag_candidate *const *d_out);
/* BM25Okapi.get_scores(query) itself: out host, n_docs fp64. */
int anrag_bm25_scores(anrag_index *idx, const int32_t *term_ids, int32_t n_terms,
                      double *out_scores);

/* ------------------------------------------------------------------ fusion
 * SearchEngine.weighted_reciprocal_rank_fusion, search_engine.py:21-34, followed
 * by the caller's truncation to common_sections_n (query_rag_retrieval.py:360-362):
 *   score[id] += weight[l] * (1 / (k + rank)), rank from 1, lists in order;
 *   stable sort by score descending (ties keep first-insertion order).
 * ids: host, the lists concatenated; list_len[l] entries each. fp64, bit-exact.
 * A negative id is padding, in every form of the kernel (one workgroup, all-pairs
 * grid, radix sorts): it occupies its rank -- the entries behind it keep theirs --
 * contributes nothing and is never returned.  1 <= n_lists <= ANRAG_WRRF_MAX_LISTS,
 * empty lists allowed. */
int anrag_wrrf(anrag_index *idx, const int64_t *ids, const int32_t *list_len,
               const double *weight, int32_t n_lists, double k, int32_t top_n, int64_t *out_id,
               double *out_score, int32_t *out_count);

/* ------------------------------------------------------------------ fused hybrid query
 * The body of retrieve_documents for one dense model + BM25
 * (query_rag_retrieval.py:197-220, :304-335, :356-378) in one call: dense scan on
 * the primary stream, BM25 on the secondary, WRRF + top-n on the device.
 * n_terms == 0 or w_bm25 <= 0 skips BM25 (then the dense list is returned, :363-366).
 * allow_* as above, one per row space.  Callers on several threads overlap: the
 * index lock is held while a call enqueues, not while it waits for its result. */
int anrag_hybrid_search(anrag_index *idx, const float *query, const int32_t *term_ids,
                        int32_t n_terms, int32_t similarity_k, double w_dense, double w_bm25,
                        double wrrf_k, int32_t top_n, const uint8_t *allow_dense,
                        int32_t n_dense_sources, const uint8_t *allow_bm25,
                        int32_t n_bm25_sources, int64_t *out_id, double *out_score,
                        int32_t *out_count);

/* anrag_hybrid_search for the fp64 query of the reference's text path (the embedding API's float64 vector,
 * search_engine.py:157, scored in fp64, :129; then query_rag_retrieval.py:197-220, :304-335, :356-378): same arguments,
 * outputs, envelope and errors.  The dense leg is the fp64 list scan of anrag_dense_search_f64, so the answer equals
 * anrag_dense_search_f64 + anrag_bm25_search + anrag_wrrf in ids and fused-score bits -- in ONE call: operands up, the
 * scan, BM25, merge + WRRF, results down on one stream behind a drained pipeline, one host wait.  Not pipelined (this
 * query sits behind a remote embedding call); the index lock is held for the whole call.
 * dim % 4 != 0 or dim > 3072 with a dense leg: ANRAG_ERR_UNSUPPORTED -- the caller composes the three calls. */
int anrag_hybrid_search_f64(anrag_index *idx, const double *query, const int32_t *term_ids,
                            int32_t n_terms, int32_t similarity_k, double w_dense, double w_bm25,
                            double wrrf_k, int32_t top_n, const uint8_t *allow_dense,
                            int32_t n_dense_sources, const uint8_t *allow_bm25,
                            int32_t n_bm25_sources, int64_t *out_id, double *out_score,
                            int32_t *out_count);

/* Same, operands in HBM, nothing syncs the host: d_out receives min(top_n,
 * distinct ids) records in fused order, *d_count that number, complete in
 * secondary-stream order (anrag_index_sync waits for all streams).
 * Back-to-back queries pipeline: the scans stay adjacent on the primary stream;
 * BM25 and the tail of query i run under the scans of the following queries.
 * Three launches per query: K1, K3 and one tail kernel (list merges + WRRF).  With the
 * dense prefilter, K1 is the shadow scan, and its threshold and rescore kernels run in
 * front of the tail on the tail's stream, under the following scans as well.
 * At most 32 queries are in flight per index: the call blocks on the HOST (never
 * on the device) until the query 32 back has finished with its buffers.
 * A corpus of at most 1 GiB on the index's own streams takes another route: the query's three launches go back to back on
 * ONE of four lane streams (no events between them) and consecutive queries rotate over the lanes (the reference's own corpus,
 * 9,609 x 384: 17 instead of 43 us per query); results are then complete behind anrag_index_sync / anrag_index_signal_stream.
 * PAIRING (anrag_set_scan_pairing).  Where the int8 prefilter answers the dense leg on the pipeline route and the index
 * runs on its own three streams, the call may return ANRAG_OK with the query HELD, not yet launched: the int8 scan takes
 * two queries through one walk of the shadow image, so two consecutive calls with the same similarity_k, weights, wrrf_k,
 * top_n and allow pointers are launched together as one group of 2.  The launch rule, per call:
 *   1. a query is held and the parameters are identical: both are launched as a group;
 *   2. a query is held and the parameters differ: the held one is launched alone, then 3;
 *   3. the latest scan launched on the index has not finished: this query is held (nothing launched now would start
 *      before that scan ends);
 *   4. otherwise the query is launched alone: one query on an idle device is never held.
 * A held query is launched by the next call of ANY other entry point that takes the index (anrag_index_sync,
 * anrag_index_signal_stream, anrag_index_wait_stream, anrag_index_set_streams, loads, searches, anrag_rank_batch, the
 * debug and profile calls, anrag_index_destroy), before that call does anything else; an error of that launch is returned
 * by that call.  Results on the index's own streams can only be observed through anrag_index_sync,
 * anrag_index_signal_stream or a host-pointer call, so a query is on the device no later than the first call that could
 * see its answer.  Operands must stay valid until then, as they must until the kernels have run.  With caller-owned
 * streams (anrag_index_set_streams) nothing is ever held. */
int anrag_hybrid_search_device(anrag_index *idx, const float *d_query, const int32_t *d_term_ids,
                               int32_t n_terms, int32_t similarity_k, double w_dense,
                               double w_bm25, double wrrf_k, int32_t top_n,
                               const uint32_t *d_allow_dense_bits,
                               const uint32_t *d_allow_bm25_bits, anrag_candidate *d_out,
                               int32_t *d_count);

/* n_queries hybrid queries from host memory in ONE call (no reference counterpart: the
 * reference's retrieval_eval.py:51-84 asks one query at a time; an evaluation run
 * holds thousands).  queries [n_queries][dim]; query q's term ids are
 * term_ids[term_offsets[q] .. term_offsets[q+1]) (term_offsets has n_queries+1
 * entries, term_offsets[0] == 0).  Operands go up once, one host sync per chunk.
 * Lists of 16 queries and more, both legs active and row numbers as document ids
 * (no doc_id arrays, bases 0), are ranked the way anrag_rank_batch ranks them: score
 * tiles that read the corpus once per 16 / 32 queries, a sort per list, the fusion in
 * LDS (1M x 768 top-10 lists: 43 us per query).  Everything else runs back to back
 * through the stream pipeline of anrag_hybrid_search_device -- the batch = 1 kernels,
 * one pass over the corpus per query (434 us).  Either way
 * out_id / out_score [n_queries][top_n] (tail -1 / -inf), out_count [n_queries];
 * each row equals what anrag_hybrid_search returns for that query, bit for bit. */
int anrag_hybrid_search_batch(anrag_index *idx, const float *queries, const int32_t *term_ids,
                              const int64_t *term_offsets, int32_t n_queries,
                              int32_t similarity_k, double w_dense, double w_bm25, double wrrf_k,
                              int32_t top_n, const uint8_t *allow_dense, int32_t n_dense_sources,
                              const uint8_t *allow_bm25, int32_t n_bm25_sources, int64_t *out_id,
                              double *out_score, int32_t *out_count);

/* ------------------------------------------------------------------ full ranking for lists of queries
 * retrieval_eval.py runs 7 of its 9 configurations with similarity_k = common_sections_n = 12000 -- "rank
 * everything" -- over ~8,000 queries each (src/retrieval_eval.py:142-143, :155-156, :366-378), one
 * retrieve_documents call per query.  This is the body of that call (src/query_rag_retrieval.py:197-370: every
 * active dense model's similarity search, the BM25 search, weighted RRF, truncation to common_sections_n) for a
 * LIST of queries, entirely on the device: score tiles, a per-(query, leg) radix select + sort, fusion over row
 * lists, one host sync per chunk of queries (rank_batch.hip).
 *
 * A LEG is one ranked list per query (the reference's `ranked_lists` entries, in the reference's order: dense models
 * first, BM25 last):
 *   kind ANRAG_LEG_DENSE  idx's dense rows, ranked by fp32 dot product with queries[q] (host, [n_queries][dim]) --
 *                         the arithmetic of anrag_dense_search, bit for bit
 *   kind ANRAG_LEG_DENSE_F64  idx's dense rows, ranked by the fp64 dot product with float64 queries: `queries` then points
 *                         at double [n_queries][dim] on the host (cast the pointer: (const float *)my_doubles; the
 *                         struct's layout is the same for every kind).  The arithmetic of anrag_dense_search_f64, bit
 *                         for bit: fp64 score tiles (K1TD) at the dimensions that have a tile kernel, one fp64 score pass
 *                         per query at the others.  A row whose score is -inf is not a candidate, as there.  Lists order
 *                         (score desc, row asc) with -0.0 == +0.0
 *   kind ANRAG_LEG_BM25   idx's BM25 rows, ranked by BM25 score of query q's term ids
 *                         term_ids[term_offsets[q] .. term_offsets[q+1]) (host); a query WITHOUT term ids has no such
 *                         leg, as the reference skips BM25 for it (src/search_engine.py:216-217)
 *   allow_source / n_sources   as for anrag_dense_search (NULL = no filter); a leg the filter empties is dropped for
 *                         that query like any empty list (query_rag_retrieval.py:213, :326)
 *   doc_of_row            host, one int64 per row of the leg: the document id of the row in an id space shared by the
 *                         legs (what the chunk-id strings are to the reference's fusion); NULL = the row number.
 *                         With two or more legs every id must lie in [0, id_space) and a leg must not name a
 *                         document twice (ANRAG_ERR_INVALID otherwise)
 *   weight                model_weights[name] (> 0; the caller leaves out legs of weight 0 as the reference does)
 * Each leg keeps its best min(similarity_k, allowed rows) rows by (score desc, row asc).  One leg: out = its first
 * top_n documents (query_rag_retrieval.py:363-366), out_score = their leg scores.  Several: weighted RRF with wrrf_k,
 * stable by first insertion (search_engine.py:21-34, fp64, bit-exact), first top_n; out_score = fused scores.
 * out_id (nullable) / out_score (nullable, needs out_id) [n_queries][top_n], tail -1 / -inf; out_count [n_queries].
 * expect_id / out_rank (nullable, together) [n_queries]: out_rank[q] = 1-based position of document expect_id[q] in
 * query q's answer, -1 if it is not there -- what retrieval_eval.py:75-82 looks for in the returned list; with
 * out_id == NULL only counts and ranks come back (an evaluation run over thousands of queries needs nothing else).
 * Legs of the three kinds may be mixed in one call.
 * Envelope: min(similarity_k, rows) <= 16384 for a dense leg, <= 13312 for a float64 dense leg or a BM25 leg, min(top_n, entries) <= 13312
 * when fusing (anrag_rank_caps); all legs on one device.  Outside it: ANRAG_ERR_INVALID -- use the per-query entry
 * points (any k). */
#define ANRAG_LEG_DENSE 0
#define ANRAG_LEG_BM25 1
#define ANRAG_LEG_DENSE_F64 2
typedef struct anrag_rank_leg {
    anrag_index *idx;
    int32_t kind;
    const float *queries; /* ANRAG_LEG_DENSE_F64: const double [n_queries][dim], cast */
    const int32_t *term_ids;
    const int64_t *term_offsets;
    const uint8_t *allow_source;
    int32_t n_sources;
    const int64_t *doc_of_row;
    double weight;
} anrag_rank_leg;
int anrag_rank_batch(const anrag_rank_leg *legs, int32_t n_legs, int32_t n_queries, int32_t similarity_k,
                     double wrrf_k, int32_t top_n, int64_t id_space, int64_t *out_id, double *out_score,
                     int32_t *out_count, const int64_t *expect_id, int32_t *out_rank);
/* Cumulative for this index: float64 queries of ANRAG_LEG_DENSE_F64 legs scored by the fp64 tile kernel (K1TD) and by
 * per-query score passes (a dimension without a tile kernel, or ANRAG_RANK_SCAN_TILES set in the environment). */
int anrag_rank_f64_tile_stats(anrag_index *idx, int64_t *tiled, int64_t *passed);
/* Largest list a dense (fp32 scores) / float64 dense, BM25 or fused (fp64 scores) ranking of anrag_rank_batch can return. */
int anrag_rank_caps(int32_t *out_k_max_fp32, int32_t *out_k_max_fp64);
/* The select behind a ranking has two forms for a segment (one query's scores of one leg, or its fused sums) longer
 * than the list cap: narrow = one workgroup per segment, right for lists of queries; wide = a segment cut into slices
 * across the whole device (a pass launch per 11-bit digit, a compaction launch, a finish launch; no host sync in
 * between), for one or a few queries over a large corpus.  Same order, same output bits.
 * mode: -1 auto (the measured gate table, anrag_rank_wide_gate; the default), 0 never, 1 wherever a segment exceeds the
 * cap.  Process-wide (anrag_rank_batch spans indexes); the environment's ANRAG_RANK_WIDE=0|1 is read once, before the
 * first call.  anrag_shard_group_rank_batch's per-shard sorts follow the same setting. */
int anrag_set_rank_wide(int32_t mode);
/* Cumulative, process-wide: segments sorted by the wide form and pass launches enqueued for them (a wide launch
 * enqueues the worst case, 6 passes for fp32 scores and 9 for fp64, whatever its segments turn out to need). */
int anrag_rank_wide_stats(int64_t *segments, int64_t *pass_launches);
/* The auto gate alone: *out_wide = 1 when a launch of n_seg segments of n scores (fp64 != 0: fp64 scores) takes the
 * wide form in auto mode. */
int anrag_rank_wide_gate(int32_t fp64, int32_t n_seg, int32_t n, int32_t *out_wide);
/* For tests (tests/test_gpu_rank_wide.py): planted score arrays through exactly the production launch path of the
 * select, on the index's primary stream and out of its rank pool; waits and copies out.  All arrays are HOST arrays.
 * keys [n_seg][key_stride] fp32 (fp64 != 0: fp64), n <= key_stride scores per segment, -inf = not a candidate; ties
 * (nullable, fp64 keys only) [n_seg][key_stride] = the tie-break words, unique inside a segment (the fused form), else
 * ties go to the lower position; seg_k (nullable) [n_seg] per-segment k, 0 = skip.  k above the list cap
 * (anrag_rank_caps) is cut to it, as anrag_rank_batch requires of its lists: kk = min(k, cap).
 * form: 0 narrow, 1 wide (where n exceeds the cap), -1 what the current mode picks.  parts: 0 lets the launcher choose
 * the number of slices P of the wide form, else P = parts; either way a slice is a multiple of 64 scores and at least
 * 4096, slice = max(4096, roundup64(ceil(n / P))), and ceil(n / slice) workgroups share a segment.
 * out_rows [n_seg][kk], out_keys (nullable) [n_seg][kk] the scores as fp64, out_count [n_seg] = min(kk, candidates);
 * entries past a segment's count come back as zero (the kernels do not write them). */
int anrag_debug_rank_select(anrag_index *idx, const void *keys, int32_t fp64, const uint32_t *ties, int32_t n_seg,
                            int64_t key_stride, int32_t n, int32_t k, const int32_t *seg_k, int32_t form, int32_t parts,
                            uint32_t *out_rows, double *out_keys, int32_t *out_count);

/* ------------------------------------------------------------------ sharded merge
 * After an all-gather of every shard's k candidates: merge n_lists sorted lists of
 * k records each into the global top-k (score desc, doc asc -- row order is
 * shard-local, doc ids are global and ascend with rows under row sharding).
 * List l starts at d_lists + l * list_stride records (list_stride >= k).
 * PRECONDITION: inside a list the records are in (score desc, doc asc) order,
 * equal scores included, padding (doc < 0) only at its tail, no NaN score (the
 * scans report a NaN dot product as +inf; +inf and ties among +inf are fine).  A
 * list is read only up to its first record that does not enter the running top
 * k, so a record behind an out-of-order one is never seen:
 * [(1.0,5),(1.0,6)] + [(1.0,8),(1.0,3)], k = 2 gives docs (5,6), not (3,5).  The
 * candidate entry points produce such lists whenever doc ids ascend with rows
 * (doc_id_base, or an ascending doc_id array); for other doc ids use a shard
 * group, which merges in shard order.  The order of the lists does not matter.
 * All device pointers; enqueued on the fusion stream. */
int anrag_merge_candidates_device(anrag_index *idx, const anrag_candidate *d_lists,
                                  int32_t n_lists, int32_t k, int64_t list_stride,
                                  anrag_candidate *d_out);
/* Both legs of a hybrid query on this shard, no fusion: d_out[0..k) = dense
 * candidates, d_out[k..2k) = BM25 candidates -- one rank's all-gather payload.
 * Dense runs on the primary stream, BM25 on the secondary; d_out is written
 * on the fusion stream, i.e. it is ready for whatever is enqueued on that
 * stream next (the all-gather).  n_terms == 0: BM25 is skipped as the reference
 * skips it for a query without tokens (search_engine.py:216-217) and the BM25 half
 * of d_out is padding (doc -1, score -inf) -- the payload keeps its 2k shape. */
int anrag_hybrid_candidates_device(anrag_index *idx, const float *d_query,
                                   const int32_t *d_term_ids, int32_t n_terms, int32_t k,
                                   const uint32_t *d_allow_dense_bits,
                                   const uint32_t *d_allow_bm25_bits, anrag_candidate *d_out);

/* The same for n_queries queries in one call: d_queries / d_term_ids / d_out are HOST
 * arrays of device pointers, n_terms a host array.  The library scans the queries in
 * groups of 8 per launch (each query still its own pass over the shard) -- at the
 * shard sizes of 8 GPUs that is worth 10-14 % over n single calls.  What the sharded
 * searcher calls once per exchange group. */
int anrag_hybrid_candidates_group_device(anrag_index *idx, const float *const *d_queries,
                                         const int32_t *const *d_term_ids,
                                         const int32_t *n_terms, int32_t n_queries, int32_t k,
                                         const uint32_t *d_allow_dense_bits,
                                         const uint32_t *d_allow_bm25_bits,
                                         anrag_candidate *const *d_out);
/* The whole global tail of a GROUP of sharded queries in ONE launch (fusion
 * stream).  d_lists is the all-gather receive buffer: shard l's slab starts at
 * d_lists + l*list_stride and holds n_queries blocks of 2k records, block q as
 * anrag_hybrid_candidates_device wrote it for query q ([0,k) dense, [k,2k)
 * BM25).  Per query and modality: merge the n_lists lists into the global
 * top-k, then weighted RRF on those global ranks + top-n
 * -> d_out + q*top_n, d_count[q].  Exchanging several in-flight queries per
 * all-gather amortises the collective's fixed cost (each query is still
 * scanned on its own: batch = 1 kernels).  PRECONDITION on every list of k
 * records: that of anrag_merge_candidates_device.  list_stride >= 2k *
 * n_queries; records outside the n_queries blocks of a slab are not read.  A
 * padding record of a merged list keeps its rank and adds nothing; d_out + q *
 * top_n is written up to d_count[q] = min(top_n, distinct docs) only. */
int anrag_merge_fuse_device(anrag_index *idx, const anrag_candidate *d_lists, int32_t n_lists,
                            int32_t k, int64_t list_stride, double w_dense, double w_bm25,
                            double wrrf_k, int32_t top_n, int32_t n_queries,
                            anrag_candidate *d_out, int32_t *d_count);
/* WRRF over two device candidate lists (dense, bm25) -> top_n on the device
 * (fusion stream).  Only the doc ids are read: a record with doc < 0 is padding
 * wherever it stands (it occupies its rank and is never returned), and the lists
 * need not be sorted.  0 < n_dense + n_bm25 <= 1024; d_out is written up to
 * *d_count = min(top_n, distinct docs) only. */
int anrag_wrrf_device(anrag_index *idx, const anrag_candidate *d_dense, int32_t n_dense,
                      const anrag_candidate *d_bm25, int32_t n_bm25, double w_dense,
                      double w_bm25, double k, int32_t top_n, anrag_candidate *d_out,
                      int32_t *d_count);

/* ------------------------------------------------------------------ device memory helpers
 * (so a pure-ctypes caller can stage operands without torch) */
int anrag_device_alloc(anrag_index *idx, int64_t bytes, void **out_ptr);
int anrag_device_free(anrag_index *idx, void *ptr);
int anrag_copy_to_device(anrag_index *idx, void *d_dst, const void *h_src, int64_t bytes);
int anrag_copy_to_host(anrag_index *idx, void *h_dst, const void *d_src, int64_t bytes);

/* ------------------------------------------------------------------ measurement
 * kernel_mask bit i set: every launch of kernel id i is bracketed by HIP events
 * on the stream it runs on (0 = profiling off).  anrag_profile_read drains them
 * (waits for the launches) and returns the summed device time and launch count
 * of one kernel id since the last reset. */
int anrag_profile_enable(anrag_index *idx, uint32_t kernel_mask);
/* Bracket only every n-th launch of each selected kernel id (default 1 = all).
 * A bracketed launch costs ~10 us of stream time (it cannot overlap the marker
 * before it), so a throughput measurement samples. */
int anrag_profile_set_sampling(anrag_index *idx, int32_t every_n);
int anrag_profile_reset(anrag_index *idx);
int anrag_profile_read(anrag_index *idx, int kernel_id, double *out_total_ms, int64_t *out_launches);
/* Queries the timed launches of a kernel carried (a K1 launch carries up to 8 when the
 * caller submits query groups): algorithmic bytes per launch = units / launches x N*D*4. */
int anrag_profile_read_units(anrag_index *idx, int kernel_id, int64_t *out_units);
/* Shape facts a caller needs for roofline arithmetic. */
int anrag_index_info(anrag_index *idx, int64_t *dense_rows, int32_t *dense_dim,
                     int64_t *bm25_docs, int64_t *bm25_postings, int64_t *hbm_bytes);
/* Device / pinned-host allocations and releases the library has made so far (process-wide; each one
 * synchronises the device).  A steady-state query loop must not move it: tests/test_gpu_no_alloc.py. */
int anrag_debug_alloc_calls(int64_t *out_calls);
/* How K3 cuts and serves the loaded BM25 corpus, for tests that aim at one kernel form (tests/test_gpu_bm25_forms.py).
 * Read-only, no wait.  n_cus: the device's compute units; part_docs / n_parts: documents per partition (the last one may
 * be shorter) and their number; form_single / form_group: the kernel form a launch of one query / of several takes,
 * 0 = 256 threads x 4 documents, 1 = 1,024 x 4 ("wide"), 2 = 256 x 16 ("tall").  Every pointer is nullable.  Without
 * BM25 data n_cus is still reported and the rest is 0. */
int anrag_debug_bm25_geometry(anrag_index *idx, int32_t *n_cus, int32_t *part_docs, int32_t *n_parts,
                              int32_t *form_single, int32_t *form_group);
/* The dense prefilter seen from outside, for tests of its score intervals (tests/test_gpu_dense_prefilter_bounds.py).
 * Both wait for the index's streams; neither allocates.
 * anrag_debug_prefilter_read: the form in use (0 off, 1 fp16, 2 int8), the scan's row geometry (a wave owns
 * rows_per_wave consecutive rows and walks them batch_rows at a time) and, each nullable, the image as built
 * (host, n_rows x dim fp16 values / int8 codes) and the per-row data (host, fp16: n_rows radii m; int8: n_rows x
 * {s_e, m1, m2, 0}). */
int anrag_debug_prefilter_read(anrag_index *idx, int32_t *out_form, int64_t *out_rows_per_wave, int32_t *out_batch_rows,
                               void *out_image, float *out_meta);
/* One shadow-scan launch and one threshold launch, as a group of 1..16 queries of the product runs them (list sets
 * 0 .. n_queries - 1, the primary stream), without the rescore.  The sets' hi rows and thresholds are first filled with
 * `sentinel` (the bits of a NaN other than 0x7FC00000, the NaN the scan stores for rows the filter rejects), so that a
 * row the scan did not write shows.  queries host [n_queries][dim]; allow_source as for anrag_dense_search;
 * out_hi host [n_queries][n_rows]: the upper bound of each row's fp32 score; out_threshold host [n_queries]: T. */
int anrag_debug_prefilter_bounds(anrag_index *idx, const float *queries, int32_t n_queries, int32_t k,
                                 const uint8_t *allow_source, int32_t n_sources, uint32_t sentinel, float *out_hi,
                                 float *out_threshold);
/* What the fp64 prefilter route derives from one float64 query, exactly as anrag_dense_search_f64 computes it, for
 * tests of the widened bound (tests/test_gpu_dense_prefilter_f64.py): out_q32 host [dim], the fp32 query the shadow
 * scan reads (read back from the device); out_w, the widening w = (||q - q32|| + gamma64 ||q||) Emax + dim 2^-1000
 * rounded upward; out_emax, the largest row norm over rows whose norm is finite and <= 2^60, rounded upward.  Needs a
 * built prefilter form.  Waits for the index's streams; after the first call it does not allocate. */
int anrag_debug_prefilter_f64(anrag_index *idx, const double *query, float *out_q32, double *out_w, double *out_emax);
/* The per-wave lists of the dense top-k seen from outside, for tests of the lists and of their merges
 * (tests/test_gpu_dense_lists.py).  Runs the list-producing half of a scan group of 1..16 queries exactly as the product
 * runs it (list sets 0 .. n_queries - 1, the primary stream, no deferred merge riding along): the fp32 scan with the
 * prefilter off, shadow scan + threshold + rescore with it on -- and no merge.  The sets' score and row blocks are first
 * filled with score_sentinel (the bits of a NaN other than 0x7FC00000) and row_sentinel (neither a row of the corpus nor
 * 0xFFFFFFFF, the row of an empty slot), so that a slot no kernel wrote shows.  Waits for the index's streams,
 * allocates nothing, and moves no statistic (prefilter counters, profile spans).
 * out_n_lists: lists per query (one per scan wave; a function of the corpus shape alone).  With out_scores and out_rows
 * both NULL only that is returned and nothing runs.  queries host [n_queries][dim]; allow_source as for
 * anrag_dense_search; out_scores host [n_queries][n_lists][64] fp32 and out_rows host [n_queries][n_lists][64]: each
 * list sorted by (score descending, row ascending), empty slots (-inf, 0xFFFFFFFF) last; only slots [0, k) are
 * specified when k < 64. */
int anrag_debug_dense_lists(anrag_index *idx, const float *queries, int32_t n_queries, int32_t k,
                            const uint8_t *allow_source, int32_t n_sources, uint32_t score_sentinel, uint32_t row_sentinel,
                            int32_t *out_n_lists, float *out_scores, uint32_t *out_rows);

/* ------------------------------------------------------------------ shard group
 * ONE corpus over several anrag_index objects in ONE process (the reference is one process: one RAGSystem for all
 * Streamlit threads, src/app.py:17-27): n_shards (1..ANRAG_GROUP_MAX_SHARDS) indexes, shard i on devices[i].  The same
 * device may appear several times ({0,0,0,0} = four shards on one GPU): a supported configuration.  Dense rows and BM25
 * documents are cut, independently, into contiguous blocks that differ by at most one row (shard i of n rows:
 * [i*(n/S) + min(i, n%S), ...)); every shard gets the GLOBAL idf / avgdl / k1 / b, so a score has the bits the single
 * index gives it.  The search entries take the arguments of their anrag_* namesakes, return what those return for ONE
 * index loaded with the same operands -- ids, counts and score bits -- and wait for their result.
 *
 * Hot route (hybrid, dense and BM25 with k <= ANRAG_FUSED_K_MAX): per exchange group of up to 8 queries every shard
 * enqueues its 2k candidate records per query (the three-stream pipeline of anrag_hybrid_candidates_group_device) into a
 * slab of its own HBM and records an event on its fusion stream; shard 0's fusion stream waits for those events and
 * runs ONE tail kernel for the group, which reads the other shards' slabs in place (peer access between distinct
 * devices, enabled at create; staged with hipMemcpyPeerAsync where the devices cannot map each other), merges each
 * modality's lists STABLY IN SHARD ORDER -- among equal scores the earlier shard, inside a shard the earlier position,
 * stays ahead: (score desc, global row asc) -- and fuses as the single index's tail does.  No host sync and no
 * collective between the shards; 4 exchange groups are in flight inside a batch call.  The steady state allocates
 * nothing (anrag_debug_alloc_calls).
 * Cold routes (k > ANRAG_FUSED_K_MAX, the fp64 query): the shards' host entry points one after the other and a stable
 * merge of their lists on the host.  Serial and untuned on purpose.
 * Ranked route (lists of queries, full ranking: anrag_shard_group_rank_batch below): every shard runs the score tiles and
 * the per-query sort of anrag_rank_batch over its own rows; the home device merges the shards' sorted lists stably in
 * shard order and runs the single index's fusion and emit.
 * Batched dense route (anrag_shard_group_dense_search with a list of queries, where the single index's own gate holds
 * on EVERY shard: 16 or more queries, k <= ANRAG_FUSED_K_MAX, dim % 32 == 0, 65,536 rows or more per shard): per chunk
 * of up to 256 queries every shard runs the K2 pass of anrag_dense_search on its primary stream into a result block of
 * its call pool and records an event; shard 0's primary stream waits for the events and runs ONE merge kernel (the same
 * shard-order rule, ranks by counting), then copies the chunk out.  One host wait per chunk, the next chunk's passes are
 * enqueued before it; a query whose survivor list overflowed on a shard is redone by the hot route above, as the single
 * index redoes it with its batch = 1 scan.  ANRAG_GROUP_BATCHED=0 at anrag_shard_group_create keeps such calls on the hot
 * route (measurements).
 * Not served: anrag_rank_batch itself (a rank leg takes an anrag_index), the ranking route of
 * anrag_hybrid_search_batch, the *_device entries, the score dumps: there is no group entry for them; a binding
 * reports ANRAG_ERR_UNSUPPORTED (a-nice-rag_amd/index.py).
 * A group is serialised by its own mutex for the whole call. */
#define ANRAG_GROUP_MAX_SHARDS 16
typedef struct anrag_shard_group anrag_shard_group;
int anrag_shard_group_create(const int32_t *devices, int32_t n_shards, anrag_shard_group **out);
int anrag_shard_group_destroy(anrag_shard_group *g);
/* Host operands.  n_shards larger than n_rows / n_docs: ANRAG_ERR_INVALID. */
int anrag_shard_group_dense_load(anrag_shard_group *g, const float *embeddings, int64_t n_rows, int32_t dim,
                                 const uint16_t *source_id, const int64_t *doc_id, int64_t doc_id_base);
int anrag_shard_group_bm25_load(anrag_shard_group *g, const int64_t *indptr, int64_t n_terms, const int32_t *post_doc,
                                const int32_t *post_tf, const double *idf, const int32_t *doc_len, int64_t n_docs,
                                double avgdl, double k1, double b, const uint16_t *source_id, const int64_t *doc_id,
                                int64_t doc_id_base);
int anrag_shard_group_hybrid_search(anrag_shard_group *g, const float *query, const int32_t *term_ids, int32_t n_terms,
                                    int32_t similarity_k, double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                                    const uint8_t *allow_dense, int32_t n_dense_sources, const uint8_t *allow_bm25,
                                    int32_t n_bm25_sources, int64_t *out_id, double *out_score, int32_t *out_count);
/* Always the pipelined batch = 1 kernels (the ranking route of anrag_hybrid_search_batch is not served). */
int anrag_shard_group_hybrid_search_batch(anrag_shard_group *g, const float *queries, const int32_t *term_ids,
                                          const int64_t *term_offsets, int32_t n_queries, int32_t similarity_k,
                                          double w_dense, double w_bm25, double wrrf_k, int32_t top_n,
                                          const uint8_t *allow_dense, int32_t n_dense_sources,
                                          const uint8_t *allow_bm25, int32_t n_bm25_sources, int64_t *out_id,
                                          double *out_score, int32_t *out_count);
int anrag_shard_group_dense_search(anrag_shard_group *g, const float *queries, int32_t n_queries, int32_t k,
                                   const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc, float *out_score,
                                   int32_t *out_count);
int anrag_shard_group_dense_search_f64(anrag_shard_group *g, const double *query, int32_t k,
                                       const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc,
                                       double *out_score, int32_t *out_count);
int anrag_shard_group_bm25_search(anrag_shard_group *g, const int32_t *term_ids, int32_t n_terms, int32_t k,
                                  const uint8_t *allow_source, int32_t n_sources, int64_t *out_doc, double *out_score,
                                  int32_t *out_count);
int anrag_shard_group_set_dense_prefilter(anrag_shard_group *g, int32_t mode); /* forwards to every shard */
int anrag_shard_group_set_batched_precision(anrag_shard_group *g, int32_t mode); /* anrag_set_batched_precision, likewise */
/* The batched dense route so far (each nullable): chunks of up to 256 queries run, queries it answered (the redone ones
 * included), queries redone by the hot route because a shard flagged them. */
int anrag_shard_group_batched_stats(anrag_shard_group *g, int64_t *passes, int64_t *queries, int64_t *redone);
int anrag_shard_group_sync(anrag_shard_group *g);
/* dense_row_lo / bm25_doc_lo (each nullable): n_shards + 1 block bounds (all 0 before the load); hbm_bytes: the shards'
 * and the group's own. */
int anrag_shard_group_info(anrag_shard_group *g, int32_t *n_shards, int64_t *dense_row_lo, int64_t *bm25_doc_lo,
                           int64_t *hbm_bytes);
/* Borrowed handle of shard i (stats, profiling, tests); it dies with the group.  Not to be used from another thread
 * while a call on the group runs: the group enqueues on the shard's streams under its own mutex. */
int anrag_shard_group_shard(anrag_shard_group *g, int32_t i, anrag_index **out);
/* Exchange groups enqueued so far and the host time (ns) spent enqueuing them -- every shard's launches, the event
 * records and waits, the tail launch; no uploads, no waiting for results --
 * but including the shards' host-side back-pressure: in a GPU-bound run it reads the GPU's time per group, and the
 * host's own cost only where the GPU never holds the host back.  scripts/measure_shard_group.py. */
int anrag_shard_group_debug_enqueue(anrag_shard_group *g, int64_t *out_groups, int64_t *out_ns);

/* anrag_rank_batch across shards: for the same operands it returns what anrag_rank_batch returns on ONE index loaded
 * with the whole corpus -- ids, counts, ranks and score bits.  A leg is a whole group (`group`) or one index (`idx`, e.g.
 * a model that is not sharded); exactly one of the two is set.  The legs of a call may sit on different groups, with
 * different shard counts, and on different devices.  doc_of_row is the map of the leg's GLOBAL rows.  The envelope is
 * anrag_rank_caps applied to the global lists: min(similarity_k, global rows) <= 16384 for a dense leg, <= 13312 for a
 * BM25 leg, the fused cut <= 13312; outside it ANRAG_ERR_INVALID.  Float64 legs (ANRAG_LEG_DENSE_F64) are not served
 * on shard groups: that kind is ANRAG_ERR_INVALID here, like any kind other than the two below.
 * Per chunk of queries and leg, shard s runs the score tiles and the per-query sort (k_s = min(similarity_k, its rows))
 * on its own primary stream out of its own grow-only scratch and records an event; the home device (leg 0's shard 0)
 * waits for the events on its stream, merges the S sorted lists of every query with ONE kernel per leg -- score desc,
 * among equal scores the earlier shard, then the earlier position: (score desc, global row asc) -- and runs the single
 * index's fusion and emit on the merged lists.  Peer lists are read in place where the home device can map them, else
 * staged with hipMemcpyPeerAsync.  One host sync per chunk; the steady state allocates nothing.
 * One leg with out_id == NULL: anrag_rank_batch counts instead of sorting; here the lists are formed all the same and
 * the rank is read from them (same ranks and counts).
 * ANRAG_RANK_CHUNK_BUDGET (bytes, measurements and tests only) replaces the 6 GiB of scratch a chunk may take, here and
 * in anrag_rank_batch. */
typedef struct anrag_group_rank_leg {
    anrag_shard_group *group;
    anrag_index *idx;
    int32_t kind; /* ANRAG_LEG_DENSE | ANRAG_LEG_BM25 */
    const float *queries;
    const int32_t *term_ids;
    const int64_t *term_offsets;
    const uint8_t *allow_source;
    int32_t n_sources;
    const int64_t *doc_of_row;
    double weight;
} anrag_group_rank_leg;
int anrag_shard_group_rank_batch(const anrag_group_rank_leg *legs, int32_t n_legs, int32_t n_queries,
                                 int32_t similarity_k, double wrrf_k, int32_t top_n, int64_t id_space, int64_t *out_id,
                                 double *out_score, int32_t *out_count, const int64_t *expect_id, int32_t *out_rank);

#ifdef __cplusplus
}
#endif
#endif /* ANRAG_H */
