/*
 * ivfpq.h — C-ABI of libivfpq.so, the MI355X (gfx950) IVF-PQ engine.
 *
 * Drop-in boundary for the IVF-PQ search path that Chameleon reaches through
 * Faiss's Python surface.  Each entry point names the
 * Faiss / Chameleon interface it replaces.  Plain pointers and sizes only;
 * host entry points take host buffers (numpy), *_device entry points take
 * device pointers plus a hipStream_t passed as void*.
 *
 * Conventions (as faiss.IndexIVFPQ):
 *   x: float32 [n][d] row-major;  D: float32 [n][k] ascending L2 distances
 *   (METRIC_L2) or descending inner products (METRIC_INNER_PRODUCT);
 *   I: int64 [n][k] labels, -1 (with distance FLT_MAX, or -FLT_MAX for inner
 *   product: the Faiss heap's neutral element) where fewer than k results
 *   exist.  Ties are ordered by label.
 * Errors: every int-returning function returns 0 on success and -1 on error;
 * ivfpq_last_error() gives the thread-local message (the Python layer raises
 * RuntimeError, as Faiss's SWIG wrapper does for FaissException).
 * Thread-safety: one mutex per handle; train/add/search serialize on it.
 * Stream ordering: a handle's device searches may be issued on different
 * streams without synchronizing.  By default each one waits (hipStreamWaitEvent)
 * for every search of the handle still in flight on another stream.  With
 * batches in flight on (ivfpq_set_inflight, or IVFPQ_INFLIGHT=1 in the
 * environment when the handle is created) searches on up to three streams
 * overlap, each in the per-stream workspace it last used; a fourth stream takes
 * over the least recently used workspace after waiting on the host for its
 * last search.
 * Results under concurrent GPU work: the same in both modes and beside other
 * kernels on the GPU.  Round 4's rare wrong rows under concurrent kernels came
 * from per-lane reads of the scan's shared bounds ("Uniform
 * bounds"; fixed in round 5, 0 of 1 046 400 stressed batches since).  Every per-wave
 * partial list the merge reads is also a set of tagged records (batch epoch +
 * slot): an entry this batch's scan did not leave there is never used -- its probe
 * is rescanned on the device by the merge -- and such events are counted
 * (ivfpq_get_repair_stats; 0 in every real search since the fix, and the concurrency
 * gates of the test suite assert it).
 * Test and diagnostic hooks (fault injection, seeded bounds, workspace dumps) are not part
 * of this drop-in surface: they are declared in ivfpq_test.h, for the test suite only.
 */
#ifndef CHAMELEON_IVFPQ_H
#define CHAMELEON_IVFPQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ivfpq_index ivfpq_index;

#define IVFPQ_METRIC_INNER_PRODUCT 0 /* faiss.METRIC_INNER_PRODUCT (beir faiss_search.py:170, 194) */
#define IVFPQ_METRIC_L2 1            /* faiss.METRIC_L2 */

/* Last error message of the calling thread ("" if none). */
const char* ivfpq_last_error(void);

/* Number of visible HIP devices (faiss.get_num_gpus, beir faiss_index.py:46). */
int ivfpq_device_count(void);

/* faiss.IndexIVFPQ(quantizer, d, nlist, M, nbits) / index_factory(d, "IVF<nlist>,PQ<M>")
 * (IVFPQ_random_dataset.py:22-24, bench_polysemous_1bn.py:272).  nbits must be 8. */
int ivfpq_create(int d, int nlist, int M, int nbits, int metric, int device, ivfpq_index** out);
int ivfpq_free(ivfpq_index* h);

/* Index.train(x)  (bench_polysemous_1bn.py:283; beir faiss_index.py FaissTrainIndex.build).
 * Lloyd k-means on the GPU: coarse (niter_coarse) then one per sub-space (niter_pq). */
int ivfpq_train(ivfpq_index* h, int64_t n, const float* x, int niter_coarse, int niter_pq, uint64_t seed);

/* Index.add(x) / add_with_ids(x, ids)  (bench_polysemous_1bn.py:343-345; beir faiss_index.py:41-42).
 * ids == NULL assigns ntotal, ntotal+1, ...  Encoding runs on the GPU. */
int ivfpq_add(ivfpq_index* h, int64_t n, const float* x, const int64_t* ids);

/* Index.add / add_with_ids with the vectors (and ids, nullable) already in HBM:
 * device pointers, on `stream` (NULL = the handle's stream).  Coarse assignment
 * on the matrix cores (the search's coarse kernels, top-1), PQ encode and the
 * merge into the device list image all run on the GPU (ivfpq_add takes the same
 * path from host buffers).  Reference: bench_gpu_1bn.py:598-658 (the 1e9 base
 * set added through the GPU index in slices).  Returns when the image is in place. */
int ivfpq_add_device(ivfpq_index* h, int64_t n, const float* x, const int64_t* ids, void* stream);

/* invlists.add_entries with precomputed (list, code, id) triples, e.g. from a
 * loaded Faiss index or another shard.  codes: uint8 [n][M]. */
int ivfpq_add_preencoded(ivfpq_index* h, int64_t n, const int64_t* list_no, const uint8_t* codes,
                         const int64_t* ids);

/* Index.reset(): drop all inverted-list entries, keep the trained quantizers. */
int ivfpq_reset(ivfpq_index* h);

/* index.nprobe = p / ParameterSpace().set_index_parameters(index, "nprobe=p")
 * (faiss_retriever.py:170-176, bench_polysemous_1bn.py:422).  Clamped to nlist at search. */
int ivfpq_set_nprobe(ivfpq_index* h, int nprobe);
int ivfpq_get_nprobe(const ivfpq_index* h);

/* Shard range: only inverted lists in [lo, hi) are stored and scanned (list-range sharding,
 * SURVEY.md §8(e); replaces IndexShards, bench_gpu_1bn.py:605-616).  Default [0, nlist). */
int ivfpq_set_list_range(ivfpq_index* h, int lo, int hi);

/* Index.search(x, k) -> (D, I)  (beir faiss_index.py:22, bench_polysemous_1bn.py:430,
 * faiss_retriever.py:254, faiss_server.py:197).  Host buffers. k <= 1024. */
int ivfpq_search(ivfpq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);

/* IndexIVF::search_preassigned(n, x, k, Iq, Dq, D, I, store_pairs=False)
 * (faiss_retriever.py:217-223) and faiss.contrib.ivf_tools.search_preassigned
 * (faiss_retriever.py:265).  Iq: int64 [n][nprobe] list ids (-1 = skip);
 * Dq: float32 [n][nprobe] coarse distances, NULL = zeros (the upstream default). */
int ivfpq_search_preassigned(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq, const float* Dq,
                             float* D, int64_t* I);

/* Device-pointer variants (inputs already resident in HBM; stream = hipStream_t, NULL = default).
 * The whole search: coarse probe, T3, fused LUT + scan + top-k. */
int ivfpq_search_device(ivfpq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream);
int ivfpq_search_preassigned_device(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                    const float* Dq, float* D, int64_t* I, void* stream);
/* FaissServer request handling in the RALM wire format: decode_request[_with_lists] +
 * retrieve / retrieve_with_lists + encode_answer (ralm/server/faiss_server.py:170-277;
 * formats ralm/retriever/serialization_utils.py:17-35, 38-94, 173-258).  Header integers
 * are big-endian int32, arrays native-order:
 *   with_lists = 0: msg = k | queries f32 [batch_size][dim]               -> search (nprobe of the index)
 *   with_lists = 1: msg = batch_size, dim, nprobe, k | queries | lists i64 [batch_size][nprobe]
 *                                                                          -> search_preassigned, Dq = NULL
 * The answer is written to `answer`: I i64 [batch_size][k] then D f32 [batch_size][k];
 * *answer_len (nullable) = batch_size * k * 12.  msg_len must equal the format's message
 * length for (batch_size, dim[, nprobe]), and the with-lists header must match them
 * (decode_request_with_lists asserts, serialization_utils.py:211-213). */
int ivfpq_serve_request(ivfpq_index* h, const uint8_t* msg, int64_t msg_len, int with_lists, int batch_size, int dim,
                        int nprobe, uint8_t* answer, int64_t answer_cap, int64_t* answer_len);

/* The inner-product tables T3 of n HBM-resident queries (1 <= n <= 16384 at M=16:
 * one 256 MB table buffer), computed on `stream` ahead of the preassigned search
 * of those queries.  *token receives the handle that search passes to
 * ivfpq_search_preassigned_tables_device, which consumes the tables (the queries
 * x must be unchanged in between).  The shard flow issues it on a side stream
 * while the coarse step and the probe all-gather run (T3 depends only on the
 * queries).  Up to three tables can be pending, so a shard loop can keep batches
 * in flight; a fourth precompute overwrites the oldest pending one (its token is
 * then rejected).  Training, set_trained and reset drop pending tables.
 * ivfpq_search_preassigned_device never uses precomputed tables.
 * Reference: IndexIVFPQ::search_preassigned's per-query precompute_list_tables
 * (bench_gpu_1bn.py:605-616 shard step). */
int ivfpq_precompute_tables_device(ivfpq_index* h, int64_t n, const float* x, void* stream, uint64_t* token);
int ivfpq_search_preassigned_tables_device(ivfpq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                           const float* Dq, float* D, int64_t* I, uint64_t token, void* stream);

/* Batches in flight (see "Stream ordering" above): 1 = device searches on different
 * streams overlap, 0 = each waits for the others (default, unless IVFPQ_INFLIGHT=1).
 * Waits for the handle's in-flight searches before switching.  Reference: the query
 * blocks streamed through one GPU index, bench_gpu_1bn.py:788-806. */
int ivfpq_set_inflight(ivfpq_index* h, int on);
int ivfpq_get_inflight(const ivfpq_index* h);
/* 1: the overlap is available (kept for callers of the r04 interface). */
int ivfpq_overlap_built(void);

/* Index checks of the merge kernels: code positions read back from partial lists
 * outside the image, partial-list lengths above k and pair ids outside the batch
 * are counted (and dropped, never dereferenced).  *out = the count since the
 * handle was created, over all its workspaces, after waiting for in-flight
 * searches.  0 on a correct run; the tests assert it. */
int ivfpq_get_error_count(ivfpq_index* h, int64_t* out);

/* Stale partial lists (see "Results under concurrent GPU work" above): *stale_reads =
 * queries (counted once per search) whose merge read an entry whose tag was not this batch's,
 * *repairs = probes the merge rescanned because of one; totals since the handle was
 * created, over all workspaces, after waiting for in-flight searches. */
int ivfpq_get_repair_stats(ivfpq_index* h, int64_t* stale_reads, int64_t* repairs);
/* The first stale-entry events (at most 64 per workspace), 8 uint32 each: merge site
 * (1 fast path, 2 full merge) | reader XCD << 8, query, list j | rank << 16, expected
 * tag, found tag (writer XCD in bits 28-31), found key bits, batch epoch, and the
 * number of system-scope re-reads until the tag was fresh (0xFFFFFFFF = never within
 * 2000; fast path: 1 = fresh at once, 0 = not).  *n_events = events copied to out
 * (out holds max_events x 8 words). */
int ivfpq_get_repair_log(ivfpq_index* h, uint32_t* out, int max_events, int* n_events);
/* Stage entry points of the same search (for per-stage timing): the coarse quantizer
 * (IndexFlatL2::search as in ralm/index_scanner/index_scanner.py:61-77) writing
 * Iq [n][nprobe] / Dq [n][nprobe]; and the per-query inner-product table T3. */
int ivfpq_coarse_device(ivfpq_index* h, int64_t n, const float* x, int64_t* Iq, float* Dq, void* stream);
/* The front half of one list-range shard step (the IndexShards step it replaces:
 * bench_gpu_1bn.py:605-616), on ONE stream: the coarse quantizer of this rank's n queries
 * x (-> Iq, Dq as ivfpq_coarse_device) and T3 of the n_tables queries x_tables of the
 * global batch (the table workgroups ride in the same launch as the key tiles at
 * nlist < 8192).  *token receives the tables for ivfpq_search_preassigned_tables_device
 * of exactly x_tables (same rules as ivfpq_precompute_tables_device); no side stream. */
int ivfpq_coarse_tables_device(ivfpq_index* h, int64_t n, const float* x, int64_t* Iq, float* Dq, int64_t n_tables,
                               const float* x_tables, void* stream, uint64_t* token);

/* Merge S sorted partial results [S][n][k] into [n][k] on the device (the IndexShards
 * merge, bench_gpu_1bn.py:605-616; host argsort merge, bench_multi_cpu_performance_OSDI.py:203-218).
 * metric: IVFPQ_METRIC_L2 (partials ascending) or IVFPQ_METRIC_INNER_PRODUCT (descending). */
int ivfpq_merge_topk_device(int S, int64_t n, int k, int metric, const float* Din, const int64_t* Iin, float* Dout,
                            int64_t* Iout, void* stream);

/* Linear pre-transform on device buffers (Faiss VectorTransform::apply for OPQMatrix /
 * LinearTransform: the "OPQ16" of "OPQ16,IVF262144,PQ16", bench_gpu_1bn.py:485-489,
 * extract_FPGA_required_data.py:162-165): y[i][j] = sum_t x[i][t] * A[j][t] (+ b[j]),
 * the sum a t-ordered fused-multiply-add chain from 0, bias added last (Faiss uses
 * sgemm, whose order BLAS leaves open; this is the order of oracle/ivfpq_oracle.c).
 * AT = A transposed, [d_in][d_out]; b nullable; x [n][d_in], y [n][d_out]. */
int ivfpq_linear_transform_device(int64_t n, int d_in, int d_out, const float* AT, const float* b, const float* x,
                                  float* y, void* stream);

/* First and second moments of device rows, the GPU half of PCAMatrix::train (beir
 * faiss_search.py:359-413; the "PCAR<dout>," front of bench_gpu_1bn.py:490-492): every
 * pointer is device memory, x [n][d] fp32, mean_out [d], scatter_out [d][d].
 * mean = the fp64 column sums over fixed row chunks, added in chunk order, divided by n and
 * rounded to fp32 once.  scatter = sum_r (x_r - mean)(x_r - mean)^T, the centred sum (not
 * Faiss's sum x x^T - n mean mean^T, which cancels in fp32), not divided by n, full and
 * exactly symmetric: the subtraction in fp32, the products accumulated on the fp32 matrix
 * cores per (tile, row chunk), the chunks' partial tiles added in chunk order.  No
 * floating-point atomics: two runs on one input return the same bits.  Any d in
 * [1, 65536]; n = 0 is an error, n = 1 gives a zero scatter.  The workspace is allocated
 * inside; the call returns once the results are in place on `stream`. */
int ivfpq_pca_moments_device(int64_t n, int d, const float* x, float* mean_out, float* scatter_out, void* stream);
/* The row chunk of the scatter (process-wide; rounded up to 32 rows): rows > 0 sets it, 0
 * (default) restores the length chosen from (n, d) alone.  The mean does not depend on it; the
 * scatter's summation order does, so a caller who needs the same bits across processes leaves
 * it alone.  The test suite uses it to reach the multi-chunk reduce with small n (declared
 * here beside ivfpq_flat_index_set_range_rows, its model, not in include/ivfpq_test.h). */
int ivfpq_pca_set_chunk_rows(int64_t rows);
/* How ivfpq_pca_moments_device splits n rows of d dimensions under that setting: chunks of
 * chunk_rows rows, tiles = the 64 x 64 upper-triangle output tiles.  Host arithmetic only.
 * n < 1 or a shape the entry point rejects is an error.  Outputs are nullable. */
int ivfpq_pca_get_plan(int64_t n, int d, int* chunks, int64_t* chunk_rows, int* tiles);

/* Per-stage device timing (the nsys stage split of MICRO_GPU_profiling/classify_stages.py:113-181,
 * measured live with HIP events recorded on the launch stream around each stage).
 * get_timing waits for the recorded events, returns per-stage sums in ms and launch counts
 * for stages {0: coarse probe, 1: inner-product table T3, 2: LUT + scan + top-k (all of it:
 * bucketing, seed pass, list scan, probe merge), 3: the list-scan kernel k_scan_lists alone
 * (list-major path; count 0 otherwise)}; both arrays hold 4 entries.  Resets.
 * on = 1: all stages; on = 2: only stage 3 (two events per batch: each recorded event
 * costs a few microseconds of stream time, so throughput runs time the list scan alone). */
int ivfpq_set_timing(ivfpq_index* h, int on);
int ivfpq_get_timing(ivfpq_index* h, double* ms, int64_t* count);

/* Accessors (extract_FPGA_required_data.py:174-248; bench_polysemous_1bn.py:368). */
int64_t ivfpq_ntotal(const ivfpq_index* h);
int ivfpq_is_trained(const ivfpq_index* h);
int ivfpq_get_dims(const ivfpq_index* h, int* d, int* nlist, int* M, int* nbits, int* metric);
int ivfpq_get_centroids(const ivfpq_index* h, float* out);  /* [nlist][d]  (quantizer.xb) */
int ivfpq_get_codebook(const ivfpq_index* h, float* out);   /* [M][256][d/M]  (pq.centroids) */
/* Install trained quantizers (e.g. from a Faiss .index or another process); builds T1 on the GPU. */
int ivfpq_set_trained(ivfpq_index* h, const float* centroids, const float* codebook);
int ivfpq_get_list_sizes(const ivfpq_index* h, int64_t* out); /* [nlist] (invlists.list_size) */
int ivfpq_get_list(const ivfpq_index* h, int list, uint8_t* codes, int64_t* ids); /* get_codes / get_ids */
/* T1 = precomputed_table [nlist][M][256] (IndexIVFPQ::precomputed_table), copied to the host. */
int ivfpq_get_precomputed_table(ivfpq_index* h, float* out);

/* faiss.write_index / read_index (bench_polysemous_1bn.py:287-290; beir faiss_index.py:29)
 * in this engine's own binary format ("CHIVFPQ1"). */
int ivfpq_save(ivfpq_index* h, const char* path);
int ivfpq_load(const char* path, int device, ivfpq_index** out);

/* Brute-force exact k-NN on the GPU: IndexFlatL2::search (metric L2; the coarse-quantizer
 * service of ralm/index_scanner/index_scanner.py:61-77) or IndexFlatIP::search (metric
 * INNER_PRODUCT; beir faiss_search.py's flat IP indexes).  Host buffers. */
int ivfpq_flat_search(int device, int d, int64_t nb, const float* xb, int64_t n, const float* x, int k, int metric,
                      float* D, int64_t* I);

/* ---- flat product quantizer: faiss.IndexPQ(d, M, nbits, metric) -------------------
 * (beir faiss_search.py:168-224 PQFaissSearch, also behind IndexPreTransform(OPQMatrix);
 * my_faiss_extract_scripts/nbits_experiments_fix_m.py:89).  No coarse quantizer and no
 * id map: every code is scanned for every query and the label of a code is its
 * position.  Tables as pq.compute_distance_tables (L2: |q_m - C_mj|^2) /
 * compute_inner_prod_tables, sums as pq_knn_search_with_tables (from 0, ascending m).
 * nbits must be 8; M in {8, 16, 32, 48, 64, 80, 96, 112, 128}; d <= 2048; k <= 1024.
 * Same conventions, errors and locking as above (one mutex per handle); device calls
 * of one handle on different streams run one after the other. */
typedef struct ivfpq_pq_index ivfpq_pq_index;

int ivfpq_pq_create(int d, int M, int nbits, int metric, int device, ivfpq_pq_index** out);
int ivfpq_pq_free(ivfpq_pq_index* h);
/* Index.train(x): sub-space m by the GPU k-means on the raw sub-vectors, seed + 1 + m. */
int ivfpq_pq_train(ivfpq_pq_index* h, int64_t n, const float* x, int niter, uint64_t seed);
/* Install a trained codebook [M][256][d/M] (pq.centroids). */
int ivfpq_pq_set_trained(ivfpq_pq_index* h, const float* codebook);
/* Index.add(x) (beir faiss_index.py FaissTrainIndex.build: chunks of 50 000): encoded on
 * the GPU and appended to the device code image, which grows geometrically. */
int ivfpq_pq_add(ivfpq_pq_index* h, int64_t n, const float* x);
/* The same with x in HBM, on `stream` (hipStream_t, NULL = default); returns when the codes are in place. */
int ivfpq_pq_add_device(ivfpq_pq_index* h, int64_t n, const float* x, void* stream);
/* Append precomputed codes uint8 [n][M] (e.g. from a loaded index file). */
int ivfpq_pq_add_codes(ivfpq_pq_index* h, int64_t n, const uint8_t* codes);
/* Index.reset(): drop the codes, keep the codebook. */
int ivfpq_pq_reset(ivfpq_pq_index* h);
/* Index.search(x, k) (beir faiss_index.py:22, k = 1000).  Queries are taken in chunks so
 * that the table workspace stays bounded. */
int ivfpq_pq_search(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);
int ivfpq_pq_search_device(ivfpq_pq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream);
int64_t ivfpq_pq_ntotal(const ivfpq_pq_index* h);
int ivfpq_pq_is_trained(const ivfpq_pq_index* h);
int ivfpq_pq_get_dims(const ivfpq_pq_index* h, int* d, int* M, int* nbits, int* metric);
int ivfpq_pq_get_codebook(const ivfpq_pq_index* h, float* out); /* [M][256][d/M] */
/* codes [i0, i0 + n) of the image, uint8 [n][M] (IndexPQ.codes) */
int ivfpq_pq_get_codes(ivfpq_pq_index* h, int64_t i0, int64_t n, uint8_t* out);

/* ---- IVF over raw vectors: faiss.IndexIVFFlat(quantizer, d, nlist, metric) ---------
 * (bench_gpu_1bn.py:575-578 and its siblings bench_gpu_1bn_SC.py:580,
 * bench_gpu_performance_OSDI.py:556, gpu_infinite_loop.py:590: an index key ending in
 * ",Flat"; bench_on_disk_performance.py:37; the exact ground truth of
 * compute_ground_truth.py:311 and generate_SYN_dataset.py:157, 285: "IVF1,Flat").
 * The coarse quantizer, its training and the probe selection are the IVF-PQ handle's;
 * the inverted lists hold the fp32 vectors themselves (code size 4 d bytes), and a
 * search computes fvec_L2sqr / fvec_inner_product of the query with every vector of
 * every probed list in Faiss's AVX order (IVFFlatScanner).  d must be a multiple of 4
 * in [4, 2048]; nlist >= 1; nprobe is clamped to nlist; k <= 1024; the index holds
 * fewer than 2^31 - 1 vectors; fp32 storage only.  Same conventions, errors and
 * locking as above (one mutex per handle); device calls of one handle on different
 * streams run one after the other.  The vectors live in HBM only. */
typedef struct ivfpq_ivfflat_index ivfpq_ivfflat_index;

int ivfpq_ivfflat_create(int d, int nlist, int metric, int device, ivfpq_ivfflat_index** out);
int ivfpq_ivfflat_free(ivfpq_ivfflat_index* h);
/* Index.train(x) (bench_gpu_1bn.py:592): the coarse k-means of ivfpq_train alone,
 * same seed rule -- the centroids equal an IVF-PQ index's for the same x, niter, seed. */
int ivfpq_ivfflat_train(ivfpq_ivfflat_index* h, int64_t n, const float* x, int niter, uint64_t seed);
/* Install trained centroids [nlist][d] (quantizer.xb, e.g. from a Faiss .index). */
int ivfpq_ivfflat_set_trained(ivfpq_ivfflat_index* h, const float* centroids);
/* Index.add(x) / add_with_ids(x, ids) (bench_gpu_1bn.py:598-658, the base set added in
 * slices).  ids == NULL assigns ntotal, ntotal+1, ...  The list is the coarse top-1 of
 * the search's coarse kernels, the stored code the vector's own bytes. */
int ivfpq_ivfflat_add(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids);
/* The same with x (and ids, nullable) in HBM, on `stream` (hipStream_t, NULL = the
 * handle's stream); returns when the vectors are in place. */
int ivfpq_ivfflat_add_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, const int64_t* ids, void* stream);
/* Index.reset(): drop the vectors, keep the centroids. */
int ivfpq_ivfflat_reset(ivfpq_ivfflat_index* h);
/* index.nprobe = p / ParameterSpace nprobe (bench_gpu_1bn.py:783-784); 1..1024, clamped to nlist at search. */
int ivfpq_ivfflat_set_nprobe(ivfpq_ivfflat_index* h, int nprobe);
int ivfpq_ivfflat_get_nprobe(const ivfpq_ivfflat_index* h);
/* Index.search(x, k) -> (D, I) (bench_gpu_1bn.py:788-806; compute_ground_truth.py:311).
 * Host buffers.  Queries are taken in chunks so that the workspace stays bounded. */
int ivfpq_ivfflat_search(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* IndexIVF::search_preassigned / faiss.contrib.ivf_tools.search_preassigned
 * (faiss_retriever.py:217-223, 265).  Iq: int64 [n][nprobe] list ids (-1 = skip; a list
 * id repeated in a row is scanned once); Dq is accepted and ignored (IVFFlatScanner
 * does not use the coarse distance). */
int ivfpq_ivfflat_search_preassigned(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                     const float* Dq, float* D, int64_t* I);
/* Device-pointer variants, launched on `stream` (hipStream_t, NULL = the default stream). */
int ivfpq_ivfflat_search_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                void* stream);
int ivfpq_ivfflat_search_preassigned_device(ivfpq_ivfflat_index* h, int64_t n, const float* x, int k,
                                            const int64_t* Iq, const float* Dq, float* D, int64_t* I, void* stream);
/* Accessors (index.ntotal, is_trained, d / nlist / metric_type, quantizer.xb). */
int64_t ivfpq_ivfflat_ntotal(const ivfpq_ivfflat_index* h);
int ivfpq_ivfflat_is_trained(const ivfpq_ivfflat_index* h);
int ivfpq_ivfflat_get_dims(const ivfpq_ivfflat_index* h, int* d, int* nlist, int* metric);
int ivfpq_ivfflat_get_centroids(const ivfpq_ivfflat_index* h, float* out); /* [nlist][d] */
int ivfpq_ivfflat_get_list_sizes(ivfpq_ivfflat_index* h, int64_t* out);    /* [nlist] (invlists.list_size) */
/* invlists.get_codes / get_ids of one list, label-sorted: vectors float32 [size][d],
 * ids int64 [size] (either nullable), copied from the device image. */
int ivfpq_ivfflat_get_list(ivfpq_ivfflat_index* h, int list, float* vectors, int64_t* ids);

/* ---- flat scalar quantizer: faiss.IndexScalarQuantizer(d, qtype, metric) -----------
 * (beir faiss_search.py:415-459 SQFaissSearch with "QT_fp16"; HNSWSQFaissSearch names
 * "QT_8bit").  No coarse quantizer and no id map: every code is scanned for every query
 * and the label of a code is its position.  Encode and decode are Faiss's scalar-build
 * formulas, every operation one fp32 rounding:
 *   QT_fp16          code = (half)x, round to nearest even;  y = (float)code
 *   QT_8bit          xi = vdiff[j] != 0 ? (x - vmin[j]) / vdiff[j] : 0, clamped to [0, 1];
 *                    code = (uint8)(int)(255.f * xi);
 *                    y = vmin[j] + (((float)code + 0.5f) / 255.0f) * vdiff[j]
 *   QT_8bit_uniform  the same with one (vmin, vdiff) pair for all dimensions
 * Training is RS_minmax with rangestat_arg = 0: vmin = the minimum, vdiff = the maximum
 * minus it, per dimension or over all entries; QT_fp16 needs none.  A distance is
 * fvec_L2sqr / fvec_inner_product in Faiss's AVX order over the decoded vector, so a
 * search equals "IVF1,Flat" over the decoded vectors.  The other quantizer types are
 * rejected by name.  d must be a multiple of 4 in [4, 2048]; k <= 1024; at most
 * 2^31 - 2 codes.  Same conventions, errors and locking as above (one mutex per
 * handle); device calls of one handle on different streams run one after the other. */
typedef struct ivfpq_sq_index ivfpq_sq_index;

/* faiss.ScalarQuantizer.QuantizerType */
#define IVFPQ_SQ_8BIT 0
#define IVFPQ_SQ_4BIT 1
#define IVFPQ_SQ_8BIT_UNIFORM 2
#define IVFPQ_SQ_4BIT_UNIFORM 3
#define IVFPQ_SQ_FP16 4
#define IVFPQ_SQ_8BIT_DIRECT 5
#define IVFPQ_SQ_6BIT 6

int ivfpq_sq_create(int d, int qtype, int metric, int device, ivfpq_sq_index** out);
int ivfpq_sq_free(ivfpq_sq_index* h);
/* Index.train(x): the minimum and maximum on the GPU (exact, so equal to any other order's). */
int ivfpq_sq_train(ivfpq_sq_index* h, int64_t n, const float* x);
/* Install sq.trained: [vmin (d), vdiff (d)] (QT_8bit), [vmin, vdiff] (QT_8bit_uniform), nothing (QT_fp16). */
int ivfpq_sq_set_trained(ivfpq_sq_index* h, const float* trained, int64_t count);
/* Index.add(x): encoded on the GPU and appended to the device code image, which grows geometrically. */
int ivfpq_sq_add(ivfpq_sq_index* h, int64_t n, const float* x);
/* The same with x in HBM, on `stream` (hipStream_t, NULL = default); returns when the codes are in place. */
int ivfpq_sq_add_device(ivfpq_sq_index* h, int64_t n, const float* x, void* stream);
/* Append precomputed codes uint8 [n][code_size] (e.g. from a loaded index file). */
int ivfpq_sq_add_codes(ivfpq_sq_index* h, int64_t n, const uint8_t* codes);
/* Index.reset(): drop the codes, keep the trained parameters. */
int ivfpq_sq_reset(ivfpq_sq_index* h);
/* Index.search(x, k) -> (D, I), host buffers / device pointers on `stream`. */
int ivfpq_sq_search(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);
int ivfpq_sq_search_device(ivfpq_sq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I, void* stream);
int64_t ivfpq_sq_ntotal(const ivfpq_sq_index* h);
int ivfpq_sq_is_trained(const ivfpq_sq_index* h);
int ivfpq_sq_get_dims(const ivfpq_sq_index* h, int* d, int* qtype, int* metric, int* code_size);
/* sq.trained: *count = its length; out (nullable) receives the values */
int ivfpq_sq_get_trained(const ivfpq_sq_index* h, float* out, int64_t* count);
/* codes [i0, i0 + n) of the image, uint8 [n][code_size] (IndexScalarQuantizer.codes) */
int ivfpq_sq_get_codes(ivfpq_sq_index* h, int64_t i0, int64_t n, uint8_t* out);
/* Index.sa_encode / sa_decode: x float32 [n][d] <-> codes uint8 [n][code_size], host buffers */
int ivfpq_sq_encode(ivfpq_sq_index* h, int64_t n, const float* x, uint8_t* codes);
int ivfpq_sq_decode(ivfpq_sq_index* h, int64_t n, const uint8_t* codes, float* x);

/* ---- IVF over scalar-quantizer codes: faiss.IndexIVFScalarQuantizer(quantizer, d, nlist,
 * qtype, metric, by_residual) -----------------------------------------------------------
 * (the "IVF<nlist>,SQ8" / "IVF<nlist>,SQfp16" factory keys; with QT_fp16 and by_residual = 0
 * what co.useFloat16 = True makes of an "IVF..,Flat" key in bench_gpu_1bn.py:575-578 and its
 * siblings bench_gpu_1bn_SC.py, bench_gpu_performance_OSDI.py, gpu_infinite_loop.py).
 * IndexIVFFlat's coarse quantizer, lists, adds and probe selection with the rows stored as
 * IndexScalarQuantizer's codes (same three types, same formulas, the others rejected by name).
 * by_residual: the codes encode x - centroid[list] (one fp32 subtraction per component, the list
 * the coarse top-1) instead of x.  A search decodes every row y of every probed list:
 *   L2   fvec_L2sqr(qr, y) in Faiss's AVX order with qr = q - centroid[list] when by_residual,
 *        else qr = q;
 *   IP   fvec_inner_product(q, y), plus the pair's coarse similarity when by_residual, as one
 *        fp32 add (IVFSQScannerIP: accu0 = coarse_dis).
 * So with by_residual = 0 a search equals IndexIVFFlat over the decoded vectors.  Training: the
 * coarse k-means of ivfpq_ivfflat_train, then RS_minmax (rangestat_arg 0) over the first 100 000
 * rows of the library's rand_perm(n, 1234) (all rows when n <= 100 000), replaced by their
 * residuals when by_residual; QT_fp16 trains no table.  d must be a multiple of 4 in [4, 2048];
 * nlist >= 1; nprobe is clamped to nlist; k <= 1024; fewer than 2^31 - 1 vectors.  Same
 * conventions, errors and locking as above (one mutex per handle); device calls of one handle
 * on different streams run one after the other.  The codes live in HBM only. */
typedef struct ivfpq_ivfsq_index ivfpq_ivfsq_index;

int ivfpq_ivfsq_create(int d, int nlist, int qtype, int metric, int by_residual, int device,
                       ivfpq_ivfsq_index** out);
int ivfpq_ivfsq_free(ivfpq_ivfsq_index* h);
/* Index.train(x): centroids as ivfpq_ivfflat_train (niter, seed), then the quantizer's table. */
int ivfpq_ivfsq_train(ivfpq_ivfsq_index* h, int64_t n, const float* x, int niter, uint64_t seed);
/* Install centroids [nlist][d] and sq.trained (count values: 2 d, 2 or 0, as ivfpq_sq_set_trained). */
int ivfpq_ivfsq_set_trained(ivfpq_ivfsq_index* h, const float* centroids, const float* sq_trained, int64_t count);
/* Index.add(x) / add_with_ids(x, ids); ids == NULL assigns ntotal, ntotal+1, ...  Assigned,
 * reduced to the residual (by_residual) and encoded on the GPU. */
int ivfpq_ivfsq_add(ivfpq_ivfsq_index* h, int64_t n, const float* x, const int64_t* ids);
/* The same with x (and ids, nullable) in HBM, on `stream` (hipStream_t, NULL = the handle's
 * stream); returns when the codes are in place. */
int ivfpq_ivfsq_add_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, const int64_t* ids, void* stream);
/* Append precomputed codes uint8 [n][code_size] to the lists `lists` [n] with labels ids
 * (nullable: sequential), e.g. the inverted lists of a loaded index file.  Host buffers. */
int ivfpq_ivfsq_add_codes(ivfpq_ivfsq_index* h, int64_t n, const int64_t* lists, const uint8_t* codes,
                          const int64_t* ids);
/* Index.reset(): drop the codes, keep the centroids and the quantizer's table. */
int ivfpq_ivfsq_reset(ivfpq_ivfsq_index* h);
int ivfpq_ivfsq_set_nprobe(ivfpq_ivfsq_index* h, int nprobe); /* 1..1024, clamped to nlist at search */
int ivfpq_ivfsq_get_nprobe(const ivfpq_ivfsq_index* h);
/* Index.search(x, k) -> (D, I), host buffers. */
int ivfpq_ivfsq_search(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);
/* IndexIVF::search_preassigned.  Iq: int64 [n][nprobe] list ids (-1 = skip; a list id repeated
 * in a row is scanned once, with the coarse value of its first column).  Dq [n][nprobe] is read
 * for the inner product with by_residual only (NULL = zeros, as faiss.contrib.ivf_tools passes);
 * otherwise it is accepted and ignored. */
int ivfpq_ivfsq_search_preassigned(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                   const float* Dq, float* D, int64_t* I);
/* Device-pointer variants, launched on `stream` (hipStream_t, NULL = the default stream). */
int ivfpq_ivfsq_search_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                              void* stream);
int ivfpq_ivfsq_search_preassigned_device(ivfpq_ivfsq_index* h, int64_t n, const float* x, int k, const int64_t* Iq,
                                          const float* Dq, float* D, int64_t* I, void* stream);
/* Accessors.  is_trained: centroids installed and (8-bit types) the quantizer's table. */
int64_t ivfpq_ivfsq_ntotal(const ivfpq_ivfsq_index* h);
int ivfpq_ivfsq_is_trained(const ivfpq_ivfsq_index* h);
int ivfpq_ivfsq_get_dims(const ivfpq_ivfsq_index* h, int* d, int* nlist, int* qtype, int* metric, int* by_residual,
                         int* code_size);
int ivfpq_ivfsq_get_centroids(const ivfpq_ivfsq_index* h, float* out); /* [nlist][d] */
/* sq.trained: *count = its length; out (nullable) receives the values */
int ivfpq_ivfsq_get_trained(const ivfpq_ivfsq_index* h, float* out, int64_t* count);
int ivfpq_ivfsq_get_list_sizes(ivfpq_ivfsq_index* h, int64_t* out); /* [nlist] (invlists.list_size) */
/* invlists.get_codes / get_ids of one list, label-sorted: codes uint8 [size][code_size], ids
 * int64 [size] (either nullable), copied from the device image. */
int ivfpq_ivfsq_get_list(ivfpq_ivfsq_index* h, int list, uint8_t* codes, int64_t* ids);

/* ---- flat binary codes: faiss.IndexBinaryFlat(d) -----------------------------------
 * (beir faiss_search.py BinaryFaissSearch: IndexBinaryFlat(dim * 8), binary_k = 1000
 * Hamming candidates, then a float re-rank).  d is in bits, a multiple of 8 in [8, 2048];
 * codes and queries are uint8 [n][d / 8].  Nothing is trained; the label of a code is its
 * position.  search returns D int32 and I int64 [n][k]: per query the k smallest
 * (hamming, label) pairs ascending, ties by label, padded with (2147483647, -1) - Faiss's
 * CMax<int32_t> neutral - where fewer than k codes exist.  Relation to Faiss: the distances
 * equal Faiss's for either value of use_heap; the labels equal use_heap = false
 * (hammings_knn_mc, which keeps the first-seen ids per distance); Faiss's default heap path
 * may keep other ties at the k-th distance and orders equal distances arbitrarily.
 * 1 <= k <= 1024; at most 2^31 - 2 codes.  The top-k is a counting select in two passes over
 * the codes (csrc/binary_flat.h).  Same conventions, errors and locking as above (one mutex
 * per handle); device calls of one handle on different streams run one after the other. */
typedef struct ivfpq_bin_index ivfpq_bin_index;

int ivfpq_bin_create(int d, int device, ivfpq_bin_index** out);
int ivfpq_bin_free(ivfpq_bin_index* h);
/* IndexBinary.reset(): drop the codes. */
int ivfpq_bin_reset(ivfpq_bin_index* h);
/* IndexBinary.add(x): appended to the device code image, which grows geometrically. */
int ivfpq_bin_add(ivfpq_bin_index* h, int64_t n, const uint8_t* x);
/* The same with x in HBM, on `stream` (hipStream_t, NULL = default); returns when the codes are in place. */
int ivfpq_bin_add_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, void* stream);
/* IndexBinary.search(x, k) -> (D, I), host buffers / device pointers on `stream`. */
int ivfpq_bin_search(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I);
int ivfpq_bin_search_device(ivfpq_bin_index* h, int64_t n, const uint8_t* x, int k, int32_t* D, int64_t* I,
                            void* stream);
int64_t ivfpq_bin_ntotal(const ivfpq_bin_index* h);
int ivfpq_bin_get_dims(const ivfpq_bin_index* h, int* d, int* code_size);
/* codes [i0, i0 + n) without the image's pad bytes, uint8 [n][code_size] (IndexBinaryFlat.xb) */
int ivfpq_bin_get_codes(ivfpq_bin_index* h, int64_t i0, int64_t n, uint8_t* out);
/* The plan of a search of nq queries for k results over ntotal codes of d bits (no handle,
 * no device call): bytes per row of the image, queries per work item, row segments and rows
 * per segment, queries per chunk of the histogram workspace.  Outputs are nullable. */
int ivfpq_bin_get_plan(int d, int64_t ntotal, int64_t nq, int k, int* stride, int* query_block, int* segments,
                       int64_t* segment_rows, int64_t* query_chunk);

/* ---- flat fp32 rows: faiss.IndexFlat(d, metric) / IndexFlatL2 / IndexFlatIP -----------
 * (beir faiss_index.py:39-42 and faiss_search.py:337 FlatIPFaissSearch; the ground truth of
 * bench_gpu_1bn.py:444-455; the coarse service of ralm/index_scanner/index_scanner.py:34-77).
 * The rows are resident in HBM, [ntotal][d] fp32, with their squared norms beside them
 * (computed once, at add); nothing is trained; the label of a row is its position.  search
 * is exact: distances, order, ties and padding are ivfpq_flat_search's bit for bit -- L2
 * max(0, (|x|^2 + |y|^2) - 2 <x, y>) ascending, inner product <x, y> descending, <x, y> one
 * ascending chain of fused multiply-adds, ties by label, (FLT_MAX | -FLT_MAX, -1) where fewer
 * than k rows exist.  A search is one fused matrix-core scan with the top-k in registers
 * (csrc/flat_scan.h; no distance reaches memory) and the merge of its partial lists.  Any
 * d >= 1; 1 <= k <= 1024; at most 2^31 - 2
 * rows.  The arguments are checked before any device call.  Same conventions, errors and
 * locking as above (one mutex per handle); device calls of one handle on different streams
 * run one after the other. */
typedef struct ivfpq_flat_index ivfpq_flat_index;

int ivfpq_flat_index_create(int device, int d, int metric, ivfpq_flat_index** out);
int ivfpq_flat_index_free(ivfpq_flat_index* h); /* free(NULL) returns 0 */
/* Index.reset(): drop the rows. */
int ivfpq_flat_index_reset(ivfpq_flat_index* h);
/* Index.add(x): appended to the device row image, which grows geometrically (O(rows added)). */
int ivfpq_flat_index_add(ivfpq_flat_index* h, int64_t n, const float* x);
/* The same with x in HBM, on `stream` (hipStream_t, NULL = default); returns when the rows are in place. */
int ivfpq_flat_index_add_device(ivfpq_flat_index* h, int64_t n, const float* x, void* stream);
/* Index.search(x, k) -> (D, I), host buffers / device pointers on `stream`. */
int ivfpq_flat_index_search(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I);
int ivfpq_flat_index_search_device(ivfpq_flat_index* h, int64_t n, const float* x, int k, float* D, int64_t* I,
                                   void* stream);
int64_t ivfpq_flat_index_ntotal(const ivfpq_flat_index* h);
int ivfpq_flat_index_get_dims(const ivfpq_flat_index* h, int* d, int* metric);
/* rows [i0, i0 + n) to the host, float [n][d] (IndexFlat.xb / reconstruct_n) */
int ivfpq_flat_index_get_rows(ivfpq_flat_index* h, int64_t i0, int64_t n, float* out);
/* Bookkeeping of the image (outputs nullable): rows copied from the host since create, rows
 * allocated, times the image was reallocated. */
int ivfpq_flat_index_get_stats(ivfpq_flat_index* h, int64_t* rows_from_host, int64_t* capacity, int64_t* reallocs);
/* The row range one scan workgroup of the fused path takes: rows > 0 sets it (rounded up to the
 * scan's row tile, kFlatTileRows of csrc/flat_scan.h), 0 (default) lets every search pick the
 * number of ranges that fills the device.  Results do not depend on it; the test suite uses it
 * to reach several ranges and several merge rounds with small shapes (include/ivfpq_test.h). */
int ivfpq_flat_index_set_range_rows(ivfpq_flat_index* h, int64_t rows);
/* The plan of a search of nq queries for k results over nb rows with that setting (no handle,
 * no device call): tile_q = the queries a scan workgroup takes (64; 16 for batches of at most
 * 16 queries and for k > 256); ranges x range_rows = the row ranges of a chunk of
 * min(nq, query_chunk) queries, S = the sorted partial lists per query in the workspace
 * (>= ranges), merged `fan` at a time in `rounds` rounds.  Outputs are nullable. */
int ivfpq_flat_index_get_plan(int64_t nq, int64_t nb, int k, int64_t set_rows, int* tile_q, int64_t* range_rows,
                              int* ranges, int* S, int* fan, int* rounds, int64_t* query_chunk);

/* ------------------------------------------------------------------------------------------
 * Stand-alone k-means (faiss.Kmeans / faiss.Clustering: bench_gpu_1bn.py:522-542
 * train_coarse_quantizer, wav2vec_cluster_faiss.py:186-203).  Lloyd iterations resident on the
 * GPU: the assignment is the flat index's fused scan at k = 1 over the centroids (first best
 * wins on ties, no distance matrix), the update adds every cluster's rows in ascending row
 * order into one fp64 chain per (cluster, dimension) -- the order of every *_train's host
 * update, so the centroids are those of oracle.kmeans bit for bit -- and the objective of an
 * iteration is the fp64 sum of its assignment's keys, reduced in a fixed order.  No
 * floating-point atomics: two runs give the same bits.  Supported pairs: L2 with
 * spherical = 0, inner product with spherical = 1 (centroids renormalised after every
 * update); create rejects any other pair and bad shapes before any device call.  Same
 * conventions, errors and locking as above.
 * ------------------------------------------------------------------------------------------ */
typedef struct ivfpq_clus ivfpq_clus;

int ivfpq_clus_create(int d, int k, int metric, int spherical, int device, ivfpq_clus** out);
int ivfpq_clus_free(ivfpq_clus* h); /* free(NULL) returns 0 */
/* nredo runs of niter iterations over the host rows x [n][d]; run r starts from the rows
 * rand_perm_prefix(n, k, seed + 15486557 r), or every run from init [k][d] (host) when it is
 * not NULL.  The run with the best final objective is kept (smallest for L2, largest for inner
 * product; ties keep the earlier run).  The rows stay in HBM across iterations when they fit
 * 8 GiB, and are streamed pass by pass in every iteration otherwise.  n >= k; niter >= 0;
 * nredo >= 1 (checked before the handle). */
int ivfpq_clus_train(ivfpq_clus* h, int64_t n, const float* x, int niter, int nredo, uint64_t seed,
                     const float* init);
/* The same with x in HBM, all device work on `stream` (hipStream_t, NULL = default); init is a
 * host pointer.  Returns when the training is complete. */
int ivfpq_clus_train_device(ivfpq_clus* h, int64_t n, const float* x, int niter, int nredo, uint64_t seed,
                            const float* init, void* stream);
int ivfpq_clus_get_centroids(ivfpq_clus* h, float* out); /* [k][d] of the kept run */
/* The kept run (outputs nullable): its iterations, obj [niter] = every iteration's objective
 * (Faiss iteration_stats[it].obj, taken before the update), nsplit [niter] = the empty clusters
 * split in that iteration's update. */
int ivfpq_clus_get_stats(ivfpq_clus* h, int* niter, double* obj, int64_t* nsplit);
/* The rows of one pass (assignment, ordering, accumulation): 0 (default) = chosen per call;
 * rows > 0 forces passes of that many rows and, for host rows, the streamed path.  Results do
 * not depend on it (the passes continue the same chains); the test suite uses it to reach
 * several passes with small inputs, as ivfpq_flat_index_set_range_rows above. */
int ivfpq_clus_set_pass_rows(ivfpq_clus* h, int64_t rows);
/* The library's generator: the first k entries of a seeded random permutation of [0, n)
 * (initial centroids, and the rows Kmeans / Clustering subsample).  No device call. */
int ivfpq_clus_rand_perm_prefix(int64_t n, int64_t k, uint64_t seed, int64_t* out);

/* ------------------------------------------------------------------------------------------
 * How the host cuts a batch into chunks ("Host-side splits").  Each getter returns
 * what the loop it names computes, from the same function: host arithmetic only, no handle, no
 * device call, outputs nullable.  The test suite uses them to assert that a batch is cut.
 * ------------------------------------------------------------------------------------------ */
/* The list scans of IndexIVFFlat and IndexIVFScalarQuantizer: S = the sorted partial lists per
 * query for k results when a query's probed lists hold at most `slots` row ranges of 4096 rows,
 * merged `fan` at a time. */
int ivfpq_ivf_get_plan(int k, int64_t slots, int* S, int* fan);
/* ... and the queries per chunk of their searches: nq, the [chunk][nlist] entries of entry_bytes
 * each (8; 12 for IndexIVFScalarQuantizer by_residual) within 256 MiB, the partial lists
 * (S * k * 24 bytes per query) within 2 GiB, and where residual queries are kept (by_residual with
 * L2) their [chunk][nprobe][d] floats within 256 MiB. */
int ivfpq_ivf_get_query_chunk(int64_t nq, int nlist, int entry_bytes, int S, int k, int nprobe, int d,
                              int resid_queries, int64_t* query_chunk);
/* The rows per pass of their adds, of IVF-PQ's, and of the scalar quantizer's training pass: the
 * [rows][nlist] coarse keys within 256 MiB (2^18 rows from nlist 8192 on), and where the pass
 * stages its rows (IndexIVFScalarQuantizer) their [rows][d] floats within 256 MiB. */
int ivfpq_ivf_get_pass_rows(int64_t n, int nlist, int d, int staged, int64_t* rows);
/* IndexScalarQuantizer's search of nq queries over nb codes: S, fan as above with
 * slots = ceil(nb / 4096), and the queries per chunk. */
int ivfpq_sq_get_plan(int64_t nq, int64_t nb, int k, int* S, int* fan, int64_t* query_chunk);
/* The rows per pass of n host rows of in_bytes each through a flat index's staging buffer
 * (add, sa_encode, sa_decode, the scalar quantizer's training). */
int ivfpq_host_get_pass_rows(int64_t n, int64_t in_bytes, int64_t* rows);
/* The queries per chunk of an IVF-PQ search (ivfpq_search and its kin) of a handle that holds
 * nloc of the nlist lists: the keys, the M * 2^nbits table entries and the buckets of a query
 * within 256 MiB, its nprobe * k * 64 bytes of partial lists within 2 GiB. */
int ivfpq_get_query_chunk(int64_t nq, int nlist, int M, int nbits, int nloc, int nprobe, int k, int64_t* query_chunk);
/* The queries per chunk of ivfpq_flat_search over nb rows. */
int ivfpq_flat_search_get_query_chunk(int64_t n, int64_t nb, int64_t* query_chunk);
/* The rows per pass of a k-means assignment to k centroids (every *_train). */
int ivfpq_kmeans_get_assign_rows(int64_t n, int k, int64_t* rows);

#ifdef __cplusplus
}
#endif

#endif /* CHAMELEON_IVFPQ_H */
