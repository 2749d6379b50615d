/*
 * grx.h -- C ABI of libgrx.so, the MI355X (gfx950) ReFeX / RolX hot-path library.
 *
 * The reference (dkaslovsky/GraphRole) is pure Python and has no FFI of its own; the seam this
 * library sits under is the pair of public classes and the graph-adapter ABC
 * (SURVEY.md section 8b).  Every entry point below names the reference lines it replaces.
 * graphrole_amd/ binds these symbols with ctypes; INTEGRATION.md shows the stub a GraphRole
 * maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes only.  Every function returns 0 on success and a
 *     negative grx_status otherwise; grx_last_error() returns a thread-local message.
 *   - Pointers named d_* are DEVICE pointers (hipMalloc'ed by the caller, by PyTorch's caching
 *     allocator, or by grx_dev_malloc).  h_* are host pointers (small tables / matrices that
 *     are consumed before the call returns).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All work is
 *     stream-ordered; nothing here synchronises unless the name says so.
 *   - Feature columns are column-major: one contiguous fp64 array of n values per column.
 *     "rows" buffers are row-major n x f (the gather source of the aggregation kernel).
 *   - Graph = CSR of the out-adjacency, rows in sorted-label order, column indices ascending in
 *     each row, int64 row_ptr[n+1], int32 col[nnz], optional fp64 w[nnz] (NULL = weight 1).
 *   - Node-range sharding: kernels that produce one value per node take [row_begin,row_end)
 *     and touch only those output rows, so a rank computes its own slice of a replicated graph.
 */
#ifndef GRX_H
#define GRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GRX_VERSION 1100         /* 0.11.0: grx_core_numbers (core number and onion layer of the sense-making measures);
                                    grx_eccentricity, grx_structural_holes, grx_weighted_distances,
                                    grx_weighted_betweenness, grx_clustering, grx_square_clustering, grx_nmf_transform and
                                    grx_truss_numbers joined later under the same number (added entry points only);
                                    so did grx_graphlet_orbits (graphlet degree vectors, orbits 0-14) and
                                    grx_neighbor_roles (the neighbour-role table of NeighborSense) and
                                    grx_similar_rows (structural similarity: exact top-k nearest rows) and
                                    grx_components / grx_reachable (connected, weak and strong components, closures) and
                                    grx_edge_betweenness / grx_weighted_edge_betweenness (edge betweenness centrality) and
                                    grx_triad_census (the triad census of a directed graph, per node and per graph)
                                    0.10.0: grx_biconnected (biconnected-component counts / articulation points of the
                                    sense-making measures)
                                    0.9.0: grx_distance_sums (closeness and harmonic centrality of the sense-making
                                    measures)
                                    0.8.0: grx_betweenness (unweighted betweenness centrality of the sense-making measures)
                                    0.7.0: node measures of RolX sense making (grx_pagerank, grx_eigenvector_centrality,
                                    grx_local_structure_measures) and grx_host_nnls; status GRX_ERR_NOT_CONVERGED */
#define GRX_MAX_BINS 128         /* upper bound on vertical-log bins (n < 2^63 gives < 70) */
#define GRX_MAX_ROLES 32         /* NMF rank limit of the device kernels: 1 .. 16 fused fp64-MFMA passes; 17 .. 32
                                    a composed update (several times the traffic), then with n_roles + features <= 480 */
#define GRX_MAX_NMF_FEATURES 480 /* NMF feature-count limit of the device kernels (fast paths: 120) */

typedef enum {
    GRX_OK = 0,
    GRX_ERR_INVALID = -1,        /* bad argument */
    GRX_ERR_HIP = -2,            /* HIP runtime error (message has hipGetErrorString) */
    GRX_ERR_WORKSPACE = -3,      /* workspace too small */
    GRX_ERR_UNSUPPORTED = -4,    /* shape outside the compiled limits */
    GRX_ERR_DEGENERATE = -5,     /* numerically degenerate input (e.g. an all-zero feature matrix) */
    GRX_ERR_NOT_CONVERGED = -6   /* a power iteration did not meet its tolerance within max_iter iterations (the
                                    iteration count is still written; networkx raises PowerIterationFailedConvergence) */
} grx_status;

/* Environment switches, each read once per process; all of them select between formulations that the tests compare
 * on the same inputs (same results), none changes what is computed:
 *   GRX_READBACK=memcpy        the few KB grx_refex_run / grx_nmf_fit read back before they decide what to launch next
 *                              go through hipMemcpyAsync + hipStreamSynchronize instead of mapped host memory and a flag
 *   GRX_BIN_BID_MIN_N=<rows>   column height from which the binning keeps 12-bit bucket ids (default 2 500 000)
 *   GRX_TRI_ROUNDS=<k>         workgroups of grx_triangle_counts = k x what fills the chip (default 4)
 *   GRX_KMEANS_*               see grx_kmeans1d below
 *   GRX_FORCE_COLLECTIVES=1    a one-rank communicator issues every exchange of the sharded path (bench.py)
 */
/* ------------------------------------------------------------------ runtime helpers ---- */
int grx_version(void);
const char *grx_last_error(void);
/* Device properties: CU count, wavefront size, gcn arch name (buf may be NULL). */
int grx_device_info(int *cu_count, int *wave_size, char *arch_buf, size_t arch_buf_len);
/* For callers without their own allocator (numpy-only hosts). */
int grx_dev_malloc(void **d_out, size_t bytes);
int grx_dev_free(void *d_ptr);
int grx_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes, void *stream);
int grx_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes, void *stream);
int grx_memset(void *d_dst, int value, size_t bytes, void *stream);
int grx_stream_sync(void *stream);
/*
 * Bulk host <-> device copies for PAGEABLE host memory (numpy arrays) at close to link rate: chunks through a ring
 * of pinned staging buffers, the host-side memcpy on a small thread pool while the next chunk is on the link.  The
 * only bulk data of the two public calls that crosses PCIe is the result table extract_features() hands to
 * extract_role_factors() (graphrole/roles/extract.py:59-93) and the edge arrays.  Synchronous on return.
 * grx_upload_i64_as_i32 narrows int64 edge arrays (numpy's default) while staging; GRX_ERR_INVALID if a value
 * does not fit.  grx_host_checksums: 64-bit content hash of each of ncols host columns (col_bytes each, a multiple
 * of 8; column c at h_base + c * stride_bytes) -- how a result table is recognised as unmodified when it comes back.
 * grx_min_value: min over the n x F entries of a feature-major device matrix (NaN if any entry is NaN): sklearn's
 * "Negative values in data passed to NMF" check (_nmf.py:283) without a host pass.
 */
int grx_download(void *h_dst, const void *d_src, size_t bytes, void *stream);
int grx_upload(void *d_dst, const void *h_src, size_t bytes, void *stream);
int grx_upload_i64_as_i32(int32_t *d_dst, const int64_t *h_src, size_t count, void *stream);
int grx_host_checksums(const void *h_base, int ncols, size_t col_bytes, size_t stride_bytes, uint64_t *h_out);
/* The index numpy's RandomState.choice(m, p = uniform) returns for its one uniform draw u -- searchsorted(cumsum(full(m,
 * 1 / m)) / total, u, 'right') -- without the three m-element arrays: the first k-means++ seed of sklearn's KMeans
 * (_kmeans.py:221) as grx_kmeans1d needs it. */
int grx_host_uniform_choice(int64_t m, double u, int64_t *index);
size_t grx_min_value_workspace_bytes(void);
int grx_min_value(int64_t n, int F, const double *d_X, int64_t ld, double *d_out, void *d_workspace,
                  size_t workspace_bytes, void *stream);

/* Stream-ordered event timing helpers (bench.py measures kernels on the launch stream). */
int grx_event_create(void **event_out);
int grx_event_destroy(void *event);
int grx_event_record(void *event, void *stream);
int grx_event_elapsed_ms(void *start, void *stop, float *ms_out);   /* synchronises on stop */

/* Launches the one-thread `grx_marker_kernel` on `stream`: a named fence in a rocprofv3 kernel trace (tests
 * delimit the product path with it, tools/step_timeline.py a step). */
int grx_trace_marker(int tag, void *stream);

/*
 * Per-kernel timing with HIP events recorded on the launch stream around every kernel launch
 * of this library (bench.py's roofline numbers).  Off by default.  Kernel ids are dense in
 * [0, grx_profile_kernel_count()); grx_profile_kernel_name gives the name rocprofv3 shows.
 * grx_profile_read synchronises on the recorded events and returns the totals since the last
 * grx_profile_reset.
 */
int grx_profile_enable(int on);
int grx_profile_enabled(void);                  /* 1 while the event profiler is on */
int grx_profile_select(uint64_t kernel_mask);   /* bit i = time kernel id i; 0 = all (default) */
int grx_profile_reset(void);
int grx_profile_kernel_count(void);
const char *grx_profile_kernel_name(int id);
int grx_profile_read(int id, double *total_ms, long long *launches);

/* ------------------------------------------------------------------ node-range sharding -- */
/*
 * NEW (the reference is single-process): one process per GPU, the graph and the
 * feature columns replicated, rank p computes node rows [h_bounds[p], h_bounds[p+1]) of every per-node
 * kernel.  A grx_comm is the transport between the ranks; the whole-loop drivers (grx_refex_run,
 * grx_nmf_fit) take one and issue their exchanges themselves, stream-ordered between the kernels.
 *
 *   grx_comm_create_rccl       RCCL over xGMI.  librccl.so.1 is resolved at run time (the copy the process
 *                              already loaded -- e.g. PyTorch's -- else the system one; GRX_RCCL_PATH overrides),
 *                              so single-GPU users carry no RCCL dependency.  Bootstrap as with NCCL: rank 0
 *                              calls grx_comm_rccl_unique_id, hands the GRX_COMM_ID_BYTES to every rank through
 *                              any channel it has (torch.distributed, MPI, a file), every rank calls create.
 *                              flags & GRX_COMM_SELF_VIA_TRANSPORT: transfers of a rank to itself go through
 *                              ncclSend / ncclRecv as well (functional test of the RCCL calls on a one-GPU box).
 *   grx_comm_create_callbacks  any other transport (the gloo-staged test transport of tests/, MPI ...): the two
 *                              primitives below as function pointers.
 * Primitives (stream-ordered; d_* are device pointers):
 *   grx_comm_all_reduce        in place over `count` elements of grx_dtype with GRX_SUM / GRX_MAX
 *   grx_comm_exchange          a group of point-to-point transfers.  Between one pair of ranks, sends and
 *                              receives are matched in the order they appear in `ops`.
 * Composites over a row partition h_bounds (host int64[world + 1]); column j of a block = base + j * ld
 * elements; rank q OWNS columns q, q + world, ... of a block.  None of them packs: every transfer reads /
 * writes the row slice of a column where it lies.
 *   grx_comm_all_gather_rows     every column (host table of device pointers) holds this rank's rows ->
 *                                complete on every rank (the next generation's gather source, W of the NMF)
 *   grx_comm_columns_to_owners   d_block [ncols x ld] with this rank's rows valid -> d_owned [n_owned x ld_owned]:
 *                                the owned columns with ALL rows (the owner bins whole columns)
 *   grx_comm_owned_to_rows       the inverse for per-column results (uint8 bins): d_owned whole owned columns
 *                                -> d_block [ncols x ld] with this rank's rows of EVERY column
 * Timing (bench.py --gpus N): grx_comm_timing(comm, 1) records HIP events around every primitive;
 * grx_comm_timing_read folds them into calls / milliseconds per kind (grx_comm_kind) and synchronises.
 */
typedef struct grx_comm grx_comm;
typedef enum { GRX_F64 = 0, GRX_I32 = 1, GRX_I64 = 2, GRX_U8 = 3 } grx_dtype;
typedef enum { GRX_SUM = 0, GRX_MAX = 1 } grx_reduce_op;
typedef enum { GRX_COMM_ALL_REDUCE = 0, GRX_COMM_EXCHANGE = 1, GRX_COMM_ALL_GATHER_ROWS = 2,
               GRX_COMM_COLUMNS_TO_OWNERS = 3, GRX_COMM_OWNED_TO_ROWS = 4, GRX_COMM_KINDS = 5 } grx_comm_kind;
typedef struct { int is_recv; int peer; void *d_ptr; size_t bytes; } grx_p2p_op;
typedef int (*grx_all_reduce_fn)(void *user, void *d_buf, size_t count, int dtype, int op, void *stream);
typedef int (*grx_exchange_fn)(void *user, int n_ops, const grx_p2p_op *ops, void *stream);
#define GRX_COMM_ID_BYTES 128
#define GRX_COMM_SELF_VIA_TRANSPORT 1
int grx_comm_rccl_unique_id(void *h_id);
int grx_comm_create_rccl(const void *h_id, int rank, int world, int flags, grx_comm **out);
int grx_comm_create_callbacks(int rank, int world, grx_all_reduce_fn all_reduce, grx_exchange_fn exchange, void *user,
                              grx_comm **out);
int grx_comm_destroy(grx_comm *comm);
int grx_comm_rank(const grx_comm *comm);
int grx_comm_world(const grx_comm *comm);
int grx_comm_all_reduce(grx_comm *comm, void *d_buf, size_t count, int dtype, int op, void *stream);
int grx_comm_exchange(grx_comm *comm, int n_ops, const grx_p2p_op *ops, void *stream);
int grx_comm_all_gather_rows(grx_comm *comm, const int64_t *h_bounds, int ncols, void *const *h_col_ptrs,
                             int elem_bytes, void *stream);
int grx_comm_columns_to_owners(grx_comm *comm, const int64_t *h_bounds, int ncols, const void *d_block, int64_t ld,
                               int elem_bytes, void *d_owned, int64_t ld_owned, void *stream);
int grx_comm_owned_to_rows(grx_comm *comm, const int64_t *h_bounds, int ncols, const void *d_owned, int64_t ld_owned,
                           int elem_bytes, void *d_block, int64_t ld, void *stream);
int grx_comm_timing(grx_comm *comm, int on);
int grx_comm_timing_read(grx_comm *comm, int kind, long long *calls, double *ms);
int grx_comm_timing_reset(grx_comm *comm);

/* ------------------------------------------------------------------ graph ingest -------- */
/*
 * Edge list -> the CSR structures of this library, on the device.  Replaces the host-side construction the
 * adapters need before anything can run (graphrole/graph/interface/networkx.py:36-46 get_nodes / get_neighbors,
 * base.py:18-26 row order): ~1 s of numpy per 10 M edges against milliseconds here.
 *   d_src / d_dst  int32[m] row indices (0..n-1 = sorted node labels); every edge once (undirected: either
 *                  orientation; a self-loop once); d_w fp64[m] or NULL.
 *   internal order: rows sorted by out-degree descending, ties by label (hub rows become a prefix):
 *                  d_perm[i] = label row of internal row i, d_inv its inverse.
 *   d_row_ptr int64[n+1], d_col int32[nnz] ascending per row, d_wcol fp64[nnz] (aligned with d_col, NULL if
 *                  unweighted), d_agg_col int32[nnz] = the same rows with the neighbours in ADJACENCY order (the
 *                  order the incident edges appear in the edge list = G[node] order of a graph built by
 *                  add_edge in that order): the summation order of grx_aggregate.
 *   nnz            2m - #self-loops (undirected) or m (directed): the caller counts the loops.
 *   directed:      d_t_row_ptr / d_t_col / d_t_w = the transposed (in-) adjacency, ascending (weighted in-degree).
 * grx_orient_count / grx_orient_fill: the degree-oriented copy for grx_triangle_counts (arc u -> v kept iff
 * (d'(u), u) < (d'(v), v), d' = degree without the self-loop) and its per-arc table; count first (o_row_ptr,
 * o_nnz = o_row_ptr[n] read back by the caller), then fill with the same workspace.
 */
size_t grx_ingest_workspace_bytes(int64_t n, int64_t m, int directed);
int grx_ingest(int64_t n, int64_t m, const int32_t *d_src, const int32_t *d_dst, const double *d_w, int directed,
               int64_t nnz, int32_t *d_perm, int32_t *d_inv, int64_t *d_row_ptr, int32_t *d_col, double *d_wcol,
               int32_t *d_agg_col, int64_t *d_t_row_ptr, int32_t *d_t_col, double *d_t_w, void *d_workspace,
               size_t workspace_bytes, void *stream);
/* out[c * ld + i] = col_c[d_index[i]] for F columns (host table of device pointers): the result table from the
 * internal row order back to label order (d_index = inv), one contiguous F x ld block for a single copy out. */
int grx_permute_columns(int64_t n, int F, const double *const *h_col_ptrs, const int32_t *d_index, double *d_out,
                        int64_t ld, void *stream);
size_t grx_orient_workspace_bytes(int64_t n);
int grx_orient_count(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, int64_t *d_o_row_ptr, void *d_workspace,
                     size_t workspace_bytes, void *stream);
int grx_orient_fill(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int64_t *d_o_row_ptr, int64_t o_nnz,
                    int32_t *d_o_col, uint64_t *d_o_arc, void *d_workspace, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ generation 0 -------- */
/*
 * Weighted row sums of a CSR.  Replaces NetworkxInterface._get_local_features
 * (graphrole/graph/interface/networkx.py:48-63): out-degree / undirected degree from the CSR,
 * in-degree from the transposed CSR.  add_self_loop != 0 adds the diagonal entry a second time
 * (networkx counts an undirected self-loop twice).  Deterministic summation order.
 */
int grx_row_sums(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                 int add_self_loop, int64_t row_begin, int64_t row_end, double *d_out,
                 void *stream);

/* out[i] = a[i] + b[i]  (total_degree = in_degree + out_degree, networkx.py:57). */
int grx_add_columns(int64_t n, const double *d_a, const double *d_b, double *d_out, void *stream);

/*
 * Ego-net features.  Replaces NetworkxInterface._get_egonet_features + _get_edge_sum
 * (graphrole/graph/interface/networkx.py:71-83,115-123).  ego(v) = {v} U row(v);
 * internal[v] = weight of edges with both ends in ego(v) (undirected: each edge and self-loop
 * once; directed: every arc); external[v] = weight of edges leaving ego(v).
 * d_rowsum: plain weighted row sums of the same CSR (grx_row_sums with add_self_loop = 0, all n
 * rows); required when d_w != NULL, ignored otherwise.
 * nnz: number of CSR entries (d_row_ptr[n]); d_workspace: grx_egonet_workspace_bytes(n, nnz) bytes of device scratch (round 5: one aligned 128-byte slot per node --
 * its row sum, where its row begins, how long it is and its first 28 ids -- so that a member of an ego set costs one
 * aligned request instead of three or four, and the lists of the rows the wavefront / workgroup kernels own).
 * Weights are read for the arcs that END inside the ego set only; what leaves it is rowsum(a) minus that, exactly 0
 * for a closed row, and added arc by arc when the difference would cancel more than six bits.
 */
size_t grx_egonet_workspace_bytes(int64_t n, int64_t nnz);
int grx_egonet_features(int64_t n, int64_t nnz, const int64_t *d_row_ptr, const int32_t *d_col,
                        const double *d_w, const double *d_rowsum, int directed,
                        int64_t row_begin, int64_t row_end, double *d_internal,
                        double *d_external, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Fast path of the same ego-net features for UNWEIGHTED UNDIRECTED graphs (BASELINE configs
 * 1-4), exact in integer arithmetic:  with d' the loop-free degrees, L the self-loop flags and
 * T(v) the number of triangles through v,
 *     internal(v) = d'(v) + T(v) + sum_{a in ego(v)} L(a),
 *     external(v) = sum_{a in ego(v)} d'(a) - 2 (d'(v) + T(v)).
 * grx_triangle_counts accumulates T (caller zero-fills d_T, uint64[n]) from the degree-oriented
 * graph (CSR that keeps arc u->v iff (d'(u),u) < (d'(v),v), columns ascending); only source rows
 * [row_begin,row_end) are processed, so ranks can split the arcs and all-reduce(SUM) d_T.
 * d_o_arc: one uint64 per oriented arc k = u->v (the arcs are the kernel's work items; the table is read sequentially
 * instead of dependent random lookups): o_row_ptr[v] | min(d+(v), 1023) << 32 | min(d+(u), 1023) << 42 |
 * min(k - o_row_ptr[u], 1023) << 52 -- where the target's own list lies and how long it is, how long the source's
 * list is and where in it the arc stands (requires o_nnz < 2^32; arcs with a field at 1023 are looked up from
 * o_row_ptr).
 * grx_egonet_unweighted then writes rows [row_begin,row_end); d_scratch: int32[n] (degree < 2^30).
 * d_hub_rows / n_hub_rows (optional): ascending rows with more than hub_degree neighbours; they get a
 * workgroup each instead of an 8-lane group.
 */
int grx_triangle_counts(int64_t n, const int64_t *d_o_row_ptr, const int32_t *d_o_col,
                        const uint64_t *d_o_arc, int64_t row_begin, int64_t row_end, uint64_t *d_T,
                        void *stream);
int grx_egonet_unweighted(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col,
                          const uint64_t *d_T, int64_t row_begin, int64_t row_end,
                          double *d_internal, double *d_external, int32_t *d_scratch,
                          const int32_t *d_hub_rows, int64_t n_hub_rows, int64_t hub_degree, void *stream);

/* ------------------------------------------------------------------ recursion ----------- */
/*
 * Pack f feature columns into the row-major gather source of grx_aggregate.
 * h_col_ptrs: HOST array of f device pointers (each an fp64 column of n values); the table
 * travels as a kernel argument, 128 columns per launch.
 * d_rows: n x ldr row-major, ldr >= f; columns f..ldr-1 are zero-filled.  grx_aggregate wants
 * ldr = grx_aggregate_ldr(f): 2, 4, 8 or a multiple of 16 doubles, so that a feature row is a
 * 16/32/64-byte slice of one cache line or a whole number of 128-byte lines.
 */
int grx_aggregate_ldr(int f);
int grx_pack_rows(int64_t n, int f, const double *const *h_col_ptrs, double *d_rows, int ldr,
                  void *stream);

/*
 * ReFeX neighbour aggregation.  Replaces RecursiveFeatureExtractor._get_next_features
 * (graphrole/features/extract.py:98-119):
 *     sum[c][v]  = sum_{u in row(v)} rows[u][c]
 *     mean[c][v] = sum[c][v] / |row(v)|      (0 when row(v) is empty)
 * BIT-EXACT with the reference: the reference evaluates every sum with Series.sum(), i.e. numpy's
 * pairwise summation over the neighbours in G[node] order (extract.py:108-113); the kernels add
 * in exactly that tree (8 interleaved accumulators, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), trailing
 * elements one by one, rows with more than 128 neighbours as a binary tree of blocks, rows with
 * more than 8192 as a running total over 8192-element chunks like ndarray.sum()).  d_col must
 * therefore list every row's neighbours in the order the reference visits them (adjacency /
 * insertion order; any order gives a correct sum, only this one gives the reference's bits).
 *
 * grx_aggregate_plan: per-graph preprocessing (lane-group width from the mean degree, block list
 * of the rows with more than 128 neighbours).  h_row_ptr is a HOST array int64[n+1].  The plan owns
 * device memory (block list + scratch); one stream at a time per plan.
 *
 * d_rows: n x ldr row-major, ldr = grx_aggregate_ldr(f), 128-byte aligned (all n rows are
 * needed: neighbours may live on any rank's slice).  A neighbour row is fetched by ldr/2
 * adjacent lanes (16 bytes each) so one request covers the whole row.
 * d_sum / d_mean: column-major, column c at d_sum + c*ld (ld >= n); only rows
 * [row_begin,row_end) are written.  Either output may be NULL.
 * grx_aggregate_minmax: column-wise minimum / maximum over the neighbours (aggs 'min' / 'max',
 * extract.py:36-47); 0 for a row without neighbours (fillna, :113).
 */
typedef struct grx_aggregate_plan grx_aggregate_plan;
int grx_aggregate_plan_create(int64_t n, const int64_t *h_row_ptr, grx_aggregate_plan **plan);
void grx_aggregate_plan_destroy(grx_aggregate_plan *plan);
int grx_aggregate_plan_info(const grx_aggregate_plan *plan, int64_t *n_long_rows, int64_t *n_blocks,
                            int *lanes_per_row);
int grx_aggregate_plan_set_lanes(grx_aggregate_plan *plan, int lanes_per_row);   /* 4, 8, 16 or 32 */
int grx_aggregate(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                  const double *d_rows, int ldr, int64_t row_begin, int64_t row_end,
                  double *d_sum, double *d_mean, int64_t ld, void *stream);
/* aggs 'var' / 'std' (pandas: sample variance, ddof = 1): with d_mean the 'mean' output of grx_aggregate for
 * the same rows, var = pairwise-sum((mean - x)^2) / (count - 1) and std = sqrt(var) -- pandas' nanvar, bit for
 * bit; 0 for rows with fewer than two neighbours (NaN -> fillna(0)).  Either output may be NULL. */
int grx_aggregate_var(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                      const double *d_rows, int ldr, int64_t row_begin, int64_t row_end, const double *d_mean,
                      double *d_var, double *d_std, int64_t ld, void *stream);
int grx_aggregate_minmax(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                         const double *d_rows, int ldr, int64_t row_begin, int64_t row_end,
                         double *d_min, double *d_max, int64_t ld, void *stream);
/*
 * The same sums / means for an INTEGER gather source: when every source column holds exact non-negative integers
 * below 2^31 (the generation-0 block of an unweighted graph: degrees and ego-net edge counts are bounded by nnz), the
 * neighbour sums are integers below 2^53 and ANY order of additions gives the bits of the reference's pairwise tree.
 * The gather source is then n x ldi int32 (ldi = grx_aggregate_ldi(f): 4 or 8, i.e. 16- / 32-byte rows instead of 32 /
 * 64): four times as many rows per cache line and per MiB of L2.  grx_aggregate_i32_ok: the plan's longest row keeps
 * max_degree * 2^31 <= 2^53 and f <= 8.  Outputs as grx_aggregate.
 */
int grx_aggregate_ldi(int f);
int grx_aggregate_i32_ok(const grx_aggregate_plan *plan, int f);
int grx_pack_rows_i32(int64_t n, int f, const double *const *h_col_ptrs, int32_t *d_rows, int ldi, void *stream);
int grx_aggregate_i32(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col, int f,
                      const int32_t *d_rows, int ldi, int64_t row_begin, int64_t row_end, double *d_sum, double *d_mean,
                      int64_t ld, void *stream);
/*
 * INTEGER feature columns with the reference's int64 semantics, 'median', 'count' / 'size' (csrc/grx_aggx.hip;
 * extract.py:26,47,111 passes any pandas-aggregatable to DataFrame.agg).
 *   grx_convert_*          switch a column between fp64 values and int64 bits (numpy astype semantics)
 *   grx_aggregate_i64      d_rows: n x ldr row-major int64 (grx_pack_rows moves bits); wrapping sum / product, min, max
 *                          over the neighbours -> int64 columns (any output may be NULL); min / max of no neighbours: 0
 *   grx_aggregate_count    number of neighbours into f columns, as fp64 values or int64 bits
 *   grx_aggregate_median   numpy's median of the neighbours' values (middle element, or (a + b) / 2 of the two middle
 *                          ones; 0 for no neighbours); workspace grx_aggregate_median_workspace_bytes(nnz of the rows)
 */
int grx_convert_i64_to_f64(int64_t n, const int64_t *d_in, double *d_out, void *stream);
int grx_convert_f64_to_i64(int64_t n, const double *d_in, int64_t *d_out, void *stream);
int grx_aggregate_i64(const int64_t *d_row_ptr, const int32_t *d_col, int f, const int64_t *d_rows, int ldr,
                      int64_t row_begin, int64_t row_end, int64_t *d_sum, int64_t *d_prod, int64_t *d_min, int64_t *d_max,
                      int64_t ld, void *stream);
int grx_aggregate_count(const int64_t *d_row_ptr, int f, int64_t row_begin, int64_t row_end, int as_i64, double *d_out,
                        int64_t ld, void *stream);
size_t grx_aggregate_median_workspace_bytes(int64_t nnz);
int grx_aggregate_median(const int64_t *d_row_ptr, const int32_t *d_col, int f, const double *d_rows, int ldr,
                         int64_t row_begin, int64_t row_end, double *d_median, int64_t ld, void *d_workspace,
                         size_t workspace_bytes, void *stream);
/* agg 'prod' (extract.py:36-47 with Series.prod): left-to-right product over the neighbours in the order
 * of d_col, 1 for a row without neighbours.  fp64 arithmetic: exact for integer columns below 2^53 (the
 * reference multiplies int64 columns in int64 and wraps silently beyond 2^63; the caller checks). */
int grx_aggregate_prod(const int64_t *d_row_ptr, const int32_t *d_col, int f, const double *d_rows, int ldr,
                       int64_t row_begin, int64_t row_end, double *d_prod, int64_t ld, void *stream);

/*
 * The whole generation loop below the ABI (single GPU).  Replaces RecursiveFeatureExtractor.extract_features /
 * _get_next_features / _update (graphrole/features/extract.py:65-142) together with FeaturePruner
 * (graphrole/features/prune.py:76-139) and the feature graph's components (graphrole/graph/graph.py:7-57):
 * generation 0 = the caller's neighbourhood-feature columns (grx_row_sums / grx_egonet_* outputs and
 * attribute columns; names as the reference spells them), then per generation: pack the retained columns,
 * aggregate over the neighbours (every aggregation of h_aggs, in that order: the candidate '<parent>(<agg>)'
 * columns are ordered aggregation-major like extract.py:158-162), bin the new columns, Chebyshev distances
 * over the working set with threshold = generation number, drop every member of a feature group but its
 * oldest, record what this generation retains (name-sorted iff something was dropped), stop when a
 * generation retains nothing or at max_generations.
 *
 * d_arena / arena_bytes: caller-provided device memory all columns, bins and scratch buffers are carved
 * from (no allocation inside); too small -> GRX_ERR_WORKSPACE with *arena_needed = bytes needed up to the
 * generation that failed (grow and call again; the run is deterministic).
 * h_columns (capacity max_columns): the RECORDED columns in record order -- generation 0's first;
 * `parent` indexes this table, names are rebuilt by the caller as name[parent] + '(' + agg + ')'.
 * h_gens (capacity max_gens >= max_generations): per-generation counts.  *generation_count = the last
 * executed generation (the reference's generation_count).  Synchronises `stream` before returning.
 *
 * h_gen0_int32 (may be NULL): per generation-0 column, non-zero if every value is an exact integer in [0, 2^31).
 * The loop then tracks what every later column IS -- an exact integer S (a neighbour sum of such a column, while
 * bits(S) + bits(longest row) <= 53), the mean fl(S / d) of one, or anything else -- learns the bit width of every
 * integer column's maximum with the read-back each generation makes anyway, and gathers generations whose parents are
 * all of the first two kinds from bit-packed rows (grx_aggregate_packed: 8 / 16 bytes per node; generations 1 and 2
 * of an unweighted graph) when only sums and means are asked for; the fall-back for integer parents whose widths are
 * not known is the int32 row of grx_aggregate_i32.  GRX_NO_PACKED_ROWS=1 (environment) switches the packed rows off.
 *
 * comm / h_bounds (NULL / NULL = one GPU): node-range sharding.  Every rank calls with the same arguments and the
 * COMPLETE generation-0 columns; it aggregates rows [h_bounds[rank], h_bounds[rank + 1]) only and the loop issues
 * its own exchanges on `stream`: candidate row slices to the column owners (grx_comm_columns_to_owners), the owners'
 * bins of the rank's rows back (grx_comm_owned_to_rows), all-reduce(MAX) of the F x F distance matrix (identical
 * pruning decisions everywhere), then the RETAINED new columns -- and only those -- completed on every rank
 * (grx_comm_all_gather_rows).  Every recorded column is complete on every rank on return; the neighbour sums
 * follow a tree that depends on the row length only, so the bits equal those of a one-GPU run.
 */
/*
 * Neighbour sums / means from BIT-PACKED integer rows.  The gather of grx_aggregate is bound by the chip's request
 * rate, and the share of requests that miss an XCD's L2 follows the BYTES of the gather table (DESIGN.md section 3,
 * profiles/r04_gather_bw.json).  On an unweighted graph every summand of generations 1 and 2
 * (graphrole/features/extract.py:104-119) is an exact integer S -- a generation-0 count or a neighbour sum of one --
 * or the mean fl(S / d) of one; a row that carries only the distinct S_k and the neighbour count d, each in the bits
 * its column maximum needs, is 8 or 16 bytes instead of 16 / 64, and the kernel rebuilds the summands in registers
 * (double(S), or double(S) / double(d): the correctly rounded division that produced the stored mean) and adds them
 * in numpy's pairwise order like grx_aggregate.  Results are bit-identical to grx_aggregate on the fp64 columns.
 *   grx_column_bits       d_bits[c] = max(d_bits[c], bits of max(column c, rows [row_begin, row_end))) for the columns
 *                         flagged in int_mask (exact non-negative integers); the caller zeroes d_bits first (the widths
 *                         of row slices combine by max, also across ranks); <= 64 columns per call
 *   grx_packed_row_bytes  8 / 16, or 0 when the fields do not fit two 64-bit words (no field straddles a word; every
 *                         field 1..62 bits, the neighbour count at most 31)
 *   grx_pack_fields       row u = fields S_k(u) = (int64) h_field_cols[k][u], then the neighbour count
 *                         d_row_ptr[u + 1] - d_row_ptr[u] when degree_bits > 0; d_rows 16-byte aligned
 *   grx_aggregate_packed  output j (column j of d_sum / d_mean, leading dimension ld) sums field out_field[j] of the
 *                         neighbours, as S or -- out_is_mean[j] -- as fl(S / d); rows of more than 128 neighbours go
 *                         through the plan's block list like grx_aggregate.  The caller guarantees
 *                         bits(S) + bits(longest row) <= 53 (sums stay exact integers).
 */
typedef struct {
    int n_fields;              /* 1 .. 7 integer source columns */
    int field_bits[8];
    int degree_bits;           /* width of the neighbour-count field, 0 = none (then no output may be a mean) */
    int n_out;                 /* 1 .. 8 outputs */
    int out_field[8];
    int out_is_mean[8];
} grx_packed_layout;
int grx_packed_row_bytes(const grx_packed_layout *layout);
int grx_column_bits(int64_t n, int ncols, const double *d_block, int64_t ld, int64_t row_begin, int64_t row_end,
                    uint64_t int_mask, int32_t *d_bits, void *stream);
int grx_pack_fields(int64_t n, const grx_packed_layout *layout, const double *const *h_field_cols, const int64_t *d_row_ptr,
                    void *d_rows, void *stream);
int grx_aggregate_packed(const grx_aggregate_plan *plan, const int64_t *d_row_ptr, const int32_t *d_col,
                         const grx_packed_layout *layout, const void *d_rows, int64_t row_begin, int64_t row_end,
                         double *d_sum, double *d_mean, int64_t ld, void *stream);

/* The pruning decision of the loop alone, on the host (no device work): FeaturePruner.prune_features given the
 * Chebyshev matrix (prune.py:76-130).  h_recorded_generation[j]: generation that recorded column j, -1 if none (a
 * new candidate); h_dist F x F; h_drop[j] = 1 for every member of a feature group but its oldest. */
int grx_host_prune(int F, const char *const *h_names, const int *h_recorded_generation, int n_generations,
                   const int32_t *h_dist, int thresh, int *h_drop);
typedef enum { GRX_AGG_SUM = 0, GRX_AGG_MEAN = 1, GRX_AGG_MIN = 2, GRX_AGG_MAX = 3, GRX_AGG_VAR = 4, GRX_AGG_STD = 5,
               GRX_AGG_PROD = 6, GRX_AGG_MEDIAN = 7, GRX_AGG_COUNT = 8, GRX_AGG_SIZE = 9 } grx_agg;
typedef struct {
    int generation;            /* generation that recorded the column */
    int parent;                /* index of the parent column in this table, -1 for generation 0 */
    int agg;                   /* grx_agg, -1 for generation 0 */
    int gen0_index;            /* index into h_gen0_cols for generation-0 columns, else -1 */
    int work_position;         /* position in the final working set (extract.py:135-141), -1 if pruned from it */
    const double *d_col;       /* fp64[n]: inside the arena, or the caller's generation-0 column */
} grx_refex_column;
typedef struct {
    int candidates, working, dropped, retained;
    int gather_row_bytes;      /* bytes per row of the generation's gather source (8 / 16: bit-packed integer rows,
                                  16 / 32: int32 rows, 8 * ldr: fp64 rows; 0 for generation 0) -- what a gather-rate
                                  ceiling has to be looked up with */
} grx_refex_generation;
/* grow (may be NULL): called when the arena is full -- returns `bytes` more bytes of device memory (256-byte aligned)
 * that stay valid as long as the caller uses the returned columns, or NULL.  With it the run never fails for want of
 * room (round 5: a first size is a guess, and a wrong guess used to cost a whole second run); columns may then lie
 * in any chunk -- d_col is an absolute pointer either way.  Without it a too-small arena is GRX_ERR_WORKSPACE and
 * *arena_needed a lower bound of what the run takes.  GRX_ERR_WORKSPACE is also what a full column table returns
 * (max_columns): a caller that grows tells the two apart by whether its grow ever returned NULL.
 * Sharded (comm != NULL): a grow that returns NULL on ONE rank (that device is out of memory) is not agreed with the
 * peers -- they wait in the next exchange until the transport's timeout ends the job. */
typedef void *(*grx_grow_fn)(size_t bytes, void *user);
/* Columns the loop hands to one call of the binning (workspace = grx_log_bin_workspace_bytes(n, this), at most about 4 GiB for
 * wide blocks of long columns; all of them for small graphs): what a caller's first arena size should assume. */
int grx_refex_bin_batch(int64_t n, int ncols);
int grx_refex_run(const grx_aggregate_plan *plan, int64_t n, const int64_t *d_row_ptr, const int32_t *d_agg_col,
                  int f0, const double *const *h_gen0_cols, const char *const *h_gen0_names, const int *h_gen0_int32,
                  int max_generations, int n_aggs, const int *h_aggs, grx_comm *comm, const int64_t *h_bounds, void *d_arena,
                  size_t arena_bytes, grx_grow_fn grow, void *grow_user, int max_columns, grx_refex_column *h_columns,
                  int *n_columns, int max_gens, grx_refex_generation *h_gens, int *generation_count, size_t *arena_needed,
                  void *stream);

/* ------------------------------------------------------------------ pruning ------------- */
/*
 * Vertical logarithmic binning of ncols columns.  Replaces vertical_log_binning
 * (graphrole/features/prune.py:13-56) as FeaturePruner._group_features applies it (:105).
 * d_cols: column j at d_cols + j*ld.  d_bins: uint8 bin ids, column j at d_bins + j*ld_bins.
 * d_nbins: int32[ncols] number of bins used per column (may be NULL).
 * Workspace: grx_log_bin_workspace_bytes(n, ncols) bytes.
 * 0 < frac < 1 (the reference raises ValueError otherwise -> GRX_ERR_INVALID).
 */
size_t grx_log_bin_workspace_bytes(int64_t n, int ncols);
int grx_vertical_log_bin(int64_t n, int ncols, const double *d_cols, int64_t ld, double frac,
                         uint8_t *d_bins, int64_t ld_bins, int32_t *d_nbins,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/* The same with a per-column representation flag (host array, may be NULL): h_is_i64[j] != 0 -- column j holds int64
 * BITS (the reference's integer columns under aggs with 'prod', see grx_aggregate_i64) and is ordered as integers:
 * np.unique on an int64 array, prune.py:27.  At most the first 512 columns of a call may be flagged. */
int grx_vertical_log_bin_typed(int64_t n, int ncols, const double *d_cols, int64_t ld, const uint8_t *h_is_i64, double frac,
                               uint8_t *d_bins, int64_t ld_bins, int32_t *d_nbins, void *d_workspace,
                               size_t workspace_bytes, void *stream);

/* Batched ascending sort of fp64 columns (the first stage of the binning; exposed for tests).
 * Workspace: grx_sort_workspace_bytes(n, ncols). */
size_t grx_sort_workspace_bytes(int64_t n, int ncols);
int grx_sort_columns(int64_t n, int ncols, const double *d_cols, int64_t ld, double *d_sorted,
                     int64_t ld_sorted, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Pairwise Chebyshev distance between binned columns.  Replaces
 * pdist(binned.T, metric='chebychev') (graphrole/features/prune.py:108).
 * h_bin_ptrs: HOST array of F device pointers to uint8 columns.  Only rows
 * [row_begin,row_end) are scanned (multi-GPU: all-reduce(MAX) the result).  d_dist: int32
 * F x F, must be zero-filled by the caller; pairs (p,q) with q >= first_new are computed
 * (first_new = 0: all pairs), the matrix is written symmetrically.  Any F: up to 96 columns are
 * one launch (one LDS tile), more are covered by one launch per pair of 48-column groups.
 * cap: the caller only needs distances up to `cap` exactly (the pruner compares with the generation
 * number, prune.py:110-113): entries <= cap are exact, larger ones are reported as SOME value > cap and
 * cost almost nothing (a pair leaves the work list once it exceeds the cap).  cap = 255: all exact.
 */
int grx_chebyshev(int64_t row_begin, int64_t row_end, int F, int first_new,
                  const uint8_t *const *h_bin_ptrs, int32_t *d_dist, int cap, void *stream);

/* ------------------------------------------------------------------ RolX NMF ------------ */
/*
 * HOST-side small dense algebra of the NNDSVDa initialisation (no device work; plain pointers to host
 * arrays, row-major).  Between its device passes (grx_gram twice, grx_project) sklearn's
 * initialisation (_nmf.py:324-359 via randomized_svd, extmath.py:531-604) only touches k x F matrices
 * with k <= F; these three calls replace ~25 numpy / LAPACK wrapper calls (0.6 ms per fit).  Any
 * F <= GRX_MAX_NMF_FEATURES: cyclic Jacobi up to 32 columns, tridiagonal QL above.
 *   grx_host_whiten        G1 = X^T X -> eigen-pairs above the numerical floor: lam_keep [k],
 *                          V_keep [F x k], T1 = V_keep / sqrt(lam_keep) [F x k]; *k = 0: X is zero
 *   grx_host_range_finder  G2 = (X T1)^T (X T1) -> T (X T orthonormal), M = (X T)^T X, randomized_svd of
 *                          M with the F x n_over test matrix omega and n_iter LU-normalised power
 *                          iterations -> Z [F x r] (U = X Z), S [r], Vt [r x F] (before svd_flip)
 *   grx_host_nndsvd_plan   per-column choices of NNDSVD from the grx_project statistics -> sign [r],
 *                          scale [r] for grx_nndsvd_apply and H [r x F] before thresholding
 */
 /* grx_host_eigh: the symmetric eigen-solver behind the two calls below (cyclic Jacobi up to 32 columns,
  * Householder tridiagonalisation + implicit QL above); h_A n x n row-major, h_w ascending, eigenvectors in
  * the columns of h_V.  Exposed for tests. */
int grx_host_eigh(int n, const double *h_A, double *h_w, double *h_V);
int grx_host_whiten(int F, const double *h_G1, double *h_T1, double *h_lam_keep, double *h_V_keep, int *k);
/* the same for a factorisation of rank r: when the plain decomposition keeps fewer than min(r, F) directions (a graded
 * table: column norms decades apart), the columns are equilibrated exactly (powers of two) before eigh */
int grx_host_whiten_for_rank(int F, const double *G1, int r, double *T1, double *lam_keep, double *V_keep, int *k_out);
int grx_host_range_finder(int F, int k, const double *h_T1, const double *h_lam_keep, const double *h_V_keep,
                          const double *h_G2, const double *h_omega, int n_over, int r, int n_iter,
                          double *h_Z, double *h_S, double *h_Vt);
int grx_host_nndsvd_plan(int r, int F, const double *h_S, const double *h_Vt, const double *h_stats,
                         double *h_sign, double *h_scale, double *h_H);
/* n < F (fewer nodes than features): sklearn's transposed randomized_svd branch (extmath.py:565-569) on the small
 * host matrix itself -- h_X n x F row-major, h_omega n x n_over; h_U n x r (before svd_flip), h_S [r], h_V r x F. */
int grx_host_small_svd(int n, int F, const double *h_X, const double *h_omega, int n_over, int r, int n_iter,
                       double *h_U, double *h_S, double *h_V);

/*
 * All NMF matrices are "feature-major": X is F x ldx (row c = feature column c, n valid
 * entries), W is r x ldw.  H is r x F row-major, HHt is r x r.  Rows [row_begin,row_end) of
 * the node axis are processed (multi-GPU: partial results are summed by the caller).
 */

/* Copy F columns given by a HOST array of device pointers into a contiguous F x ld matrix (F <= 128). */
int grx_gather_columns(int64_t n, int F, const double *const *h_col_ptrs, double *d_out,
                       int64_t ld, void *stream);

/*
 * G = (X T)^T (X T), T = h_T (host, F x k row-major; NULL = identity, k = F), k <= 128.
 * Also returns sum of all entries of X in d_out[k*k] (for X.mean()).  d_out: fp64 [k*k + 1].
 * Used for the rank-revealing orthogonal factorisation behind the NNDSVDa initialisation that
 * sklearn's NMF(init='nndsvda') performs (sklearn/decomposition/_nmf.py:316-359,
 * sklearn/utils/extmath.py:531-604) at graphrole/roles/factor.py:19.
 */
size_t grx_gram_workspace_bytes(int64_t n, int k);
int grx_gram(int64_t n, int F, const double *d_X, int64_t ldx, int64_t row_begin, int64_t row_end,
             const double *h_T, int k, double *d_out, void *d_workspace, size_t workspace_bytes,
             void *stream);

/*
 * U = X Z (Z = h_Z host, F x r row-major) written feature-major to d_U (r x ldu), plus per
 * column j statistics in d_stats (fp64 [r*4]): {max|U_j| entry with its sign, index of it,
 * sum of squares of positive part, sum of squares of negative part}.
 */
size_t grx_project_workspace_bytes(int64_t n, int r);
int grx_project(int64_t n, int F, const double *d_X, int64_t ldx, int64_t row_begin,
                int64_t row_end, const double *h_Z, int r, double *d_U, int64_t ldu,
                double *d_stats, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * NNDSVDa column transform (sklearn/decomposition/_nmf.py:324-359), in place on d_U:
 *   W[j][i] = scale[j] * max(sign[j] * U[j][i], 0)   (column 0: scale*|U|),
 *   values < eps -> 0 -> fill.   h_sign: +1/-1 per column (0 = take |.|).
 */
int grx_nndsvd_apply(int64_t n, int r, double *d_U, int64_t ldu, int64_t row_begin,
                     int64_t row_end, const double *h_sign, const double *h_scale, double eps,
                     double fill, void *stream);

/*
 * Multiplicative-update state.  Replaces the loop body of sklearn's
 * _fit_multiplicative_update (sklearn/decomposition/_nmf.py:831-868) reached from
 * graphrole/roles/factor.py:24:
 *     W <- W * (X H^T) / (W (H H^T));   H <- H * (W^T X) / ((W^T W) H);   zero denominators
 *     are replaced by float32 eps (_nmf.py:39,632,720).
 * grx_nmf_w_pass   : updates W rows [row_begin,row_end) in place and writes this rank's
 *                    partial sums  d_AB = [ W'^T X (r x F) | W'^T W' (r x r) ].
 * grx_nmf_h_update : H <- H * A / (B H) from the (all-reduced) d_AB.
 * grx_nmf_residual : d_out[0] = sum_i ||x_i - w_i H||^2 over the row range
 *                    (_beta_divergence, _nmf.py:120-133, before the square root).
 */
size_t grx_nmf_workspace_bytes(int64_t n, int F, int r);
/* grx_nmf_w_pass_next: the W pass of the NEXT iteration with the H update of the previous one folded in --
 * H = d_H_prev * A / (B d_H_prev) from the (all-reduced) d_AB_prev is computed in the kernel's prologue, used for the
 * pass and stored in d_H_out (a different buffer); equal to grx_nmf_h_update followed by grx_nmf_w_pass, one launch
 * fewer per iteration.  d_AB_prev may be d_AB (it is read before the partial sums are reduced into d_AB). */
int grx_nmf_w_pass_next(int64_t n, int F, int r, const double *d_X, int64_t ldx, double *d_W, int64_t ldw,
                        int64_t row_begin, int64_t row_end, const double *d_H_prev, const double *d_AB_prev,
                        double *d_H_out, double *d_AB, void *d_workspace, size_t workspace_bytes, void *stream);
int grx_nmf_w_pass(int64_t n, int F, int r, const double *d_X, int64_t ldx, double *d_W,
                   int64_t ldw, int64_t row_begin, int64_t row_end, const double *d_H,
                   double *d_AB, void *d_workspace, size_t workspace_bytes, void *stream);
int grx_nmf_h_update(int F, int r, double *d_H, const double *d_AB, void *stream);
int grx_nmf_residual(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *d_W,
                     int64_t ldw, int64_t row_begin, int64_t row_end, const double *d_H,
                     double *d_out, void *d_workspace, size_t workspace_bytes, void *stream);
/*
 * MDL error cost of an (encoded) factor pair: generalised KL divergence of X from W H over the
 * non-zero entries of X (graphrole/roles/description_length.py:44-61), rows [row_begin,row_end).
 * d_out[0] receives the sum.  Workspace as for the other NMF passes.
 */
int grx_nmf_kl_cost(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *d_W,
                    int64_t ldw, int64_t row_begin, int64_t row_end, const double *d_H, double *d_out,
                    void *d_workspace, size_t workspace_bytes, void *stream);
/*
 * Enqueue `iters` full single-GPU iterations followed (d_err != NULL) by one residual evaluation into
 * d_err[0]; no host synchronisation.  Same results as `iters` x (grx_nmf_w_pass, grx_nmf_h_update), two
 * launches per iteration instead of three: for F <= 120 the H update of an iteration runs in the prologue of the
 * next W pass (two scratch copies of H at the end of the workspace), d_H holds the final H on completion.
 */
int grx_nmf_iterate(int64_t n, int F, int r, const double *d_X, int64_t ldx, double *d_W,
                    int64_t ldw, double *d_H, double *d_AB, double *d_err, int iters,
                    void *d_workspace, size_t workspace_bytes, void *stream);
/* The same block of iterations on a row shard: W rows [row_begin,row_end) are updated, the partial sums of every
 * pass are summed over the ranks of `comm` (NULL: no exchange) before the H update that consumes them -- one
 * small all-reduce per iteration, enqueued between the launches.  H ends identical on every rank. */
int grx_nmf_iterate_rows(int64_t n, int F, int r, const double *d_X, int64_t ldx, double *d_W, int64_t ldw,
                         int64_t row_begin, int64_t row_end, double *d_H, double *d_AB, int iters, grx_comm *comm,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * The whole factorisation below the ABI.  Replaces get_nmf_decomposition (graphrole/roles/factor.py:10-26),
 * i.e. sklearn NMF(n_components=r, solver='mu', init='nndsvda').fit_transform(X) with its defaults
 * (tol 1e-4, max_iter 200; sklearn/decomposition/_nmf.py:1538-1553), on a feature-major device matrix:
 *   grx_nmf_init  NNDSVDa start (_nmf.py:316-359 via randomized_svd, extmath.py:531-604): two Gram
 *                 passes, the k x F host algebra (grx_host_*), one projection pass, the element-wise
 *                 transform.  h_omega: the F x n_over Gaussian test matrix the caller drew exactly like
 *                 sklearn does (global numpy RNG, n_over = r + 10).  Needs n >= F >= r.  Writes W0 to d_W
 *                 (r x ldw), H0 to d_H (r x F, device) and ||X||_F^2 to *x_sq_norm.
 *                 GRX_ERR_DEGENERATE: X is numerically zero.
 *   grx_nmf_mu    multiplicative updates from the W, H in place with sklearn's stopping rule
 *                 (_nmf.py:815-885: error every 10 iterations, stop when (prev - err) / err_init < tol).
 *                 x_sq_norm > 0 lets the convergence checks use ||X||^2 - 2<W^T X, H> + <W^T W, H H^T>
 *                 from the W-pass outputs whenever the relative squared residual exceeds 1e-8 (direct pass
 *                 over X otherwise; x_sq_norm <= 0: always direct).
 *   grx_nmf_fit   both.
 * Kernels are enqueued on `stream`; the calls synchronise it at every small read-back (three in the
 * initialisation, one per ten iterations) and return with the results complete in d_W / d_H.
 * comm / h_bounds (NULL / NULL = one GPU): row-sharded fit.  Every rank holds the same X and passes the same
 * omega; the O(n) passes cover rows [h_bounds[rank], h_bounds[rank + 1]) and the drivers issue the exchanges:
 * all-reduce(SUM) of the two Gram matrices, the projection statistics of every rank merged on the host, one
 * all-reduce of [W^T X | W^T W] per iteration (grx_nmf_iterate_rows), of the residual at direct convergence
 * checks; grx_nmf_mu / grx_nmf_fit finish by completing W on every rank (grx_comm_all_gather_rows).  H and n_iter
 * are identical on every rank.
 */
typedef struct {
    int n_iter;               /* executed iterations: sklearn's n_iter_ */
    int direct_residuals;     /* convergence checks that needed the direct ||X - W H|| pass */
    double err_init;          /* ||X - W0 H0||_F */
    double err_last;          /* error at the last convergence check */
    double x_sq_norm;         /* ||X||_F^2 as used by the checks */
} grx_nmf_info;
size_t grx_nmf_fit_workspace_bytes(int64_t n, int F, int r);
int grx_nmf_init(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *h_omega, int n_over,
                 double *d_W, int64_t ldw, double *d_H, double *x_sq_norm, grx_comm *comm, const int64_t *h_bounds,
                 void *d_workspace, size_t workspace_bytes, void *stream);
int grx_nmf_mu(int64_t n, int F, int r, const double *d_X, int64_t ldx, double *d_W, int64_t ldw, double *d_H,
               double x_sq_norm, double tol, int max_iter, grx_nmf_info *info, grx_comm *comm, const int64_t *h_bounds,
               void *d_workspace, size_t workspace_bytes, void *stream);
int grx_nmf_fit(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *h_omega, int n_over,
                double tol, int max_iter, double *d_W, int64_t ldw, double *d_H, grx_nmf_info *info, grx_comm *comm,
                const int64_t *h_bounds, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * Role transfer: the memberships of the rows of a NEW table under a fitted role x feature factor that stays fixed.
 * Replaces model.transform(X) of the sklearn NMF(solver='mu') behind graphrole/roles/factor.py:19, i.e.
 * _fit_transform(X, H=components_, update_H=False) (sklearn/decomposition/_nmf.py) for the Frobenius loss:
 * W0 = sqrt(X.mean() / r) everywhere, W <- W * (X H^T) / (W H H^T) with zero denominators replaced by float32 eps,
 * ||X - W H||_F every 10 iterations, stop when (prev - err) / err_init < tol (err_init at W0); a last block shorter
 * than 10 iterations ends without a check, tol = 0 runs max_iter iterations.
 *   d_X   feature-major F x ldx device table (non-negative), as the fit reads it;  h_H  r x F row-major on the HOST;
 *   d_W   r x ldw device output (rows >= n of a column are left alone);  info as for grx_nmf_mu (direct_residuals:
 *   checks where ||X||^2 - 2<W, X H^T> + <W^T W, H H^T> cancelled -- a relative squared residual <= 1e-8 -- and the
 *   direct grx_nmf_residual pass ran instead).
 * X is read twice (sum(X) and ||X||^2 in one pass, X H^T through grx_project) and never inside the loop: a block of up
 * to ten updates is ONE launch that keeps a row's r values of X H^T and of W in registers and H H^T in LDS.  The error
 * terms are summed in a fixed order (no floating-point atomics): two calls give the same bits.  The call synchronises
 * the stream once before the loop and once per checked block, and returns with d_W complete.
 * Limits as for the fit (1 <= r <= GRX_MAX_ROLES, F <= GRX_MAX_NMF_FEATURES, r + F <= GRX_MAX_NMF_FEATURES above 16
 * roles: GRX_ERR_UNSUPPORTED); bad arguments are GRX_ERR_INVALID before any HIP call.  n = 0 returns at once; an
 * all-zero table returns W = 0 with n_iter = max_iter (sklearn's 0 / 0 comparison never stops).  A zero row of X gives a
 * zero row of W; a zero row of H (a dead role) a zero column of W after the first update.
 */
size_t grx_nmf_transform_workspace_bytes(int64_t n, int F, int r);
int grx_nmf_transform(int64_t n, int F, int r, const double *d_X, int64_t ldx, const double *h_H, double tol,
                      int max_iter, double *d_W, int64_t ldw, grx_nmf_info *info, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ RolX encode --------- */
/*
 * 1-D Lloyd-Max quantiser.  Replaces encode() (graphrole/roles/factor.py:29-49: sklearn KMeans on
 * the flattened factor entries, every entry replaced by its cluster centre).  Deterministic:
 * sort -> prefix sums -> exact DP over <= 1024 equal cbrt-density micro-cells -> Lloyd refinement
 * -> assignment.  d_values / d_quantized: fp64[m]; d_centers: fp64[n_bins] (ascending);
 * d_info: int32[3] = {Lloyd iterations, non-empty cells, distinct output values}.  Up to 256 levels the start
 * is the exact DP; 257..65536 levels (9..16 bits: roles/extract.py:72 asks for 2**int(log2(n_roles * min(shape)))
 * on wide tables) start from the companding partition itself (equal cbrt-density cells).
 * n_bins > m is the reference's ValueError (sklearn: "n_samples=.. should be >= n_clusters=..")
 * -> GRX_ERR_INVALID.
 */
size_t grx_lloyd_max_workspace_bytes(int64_t m);
int grx_lloyd_max(int64_t m, const double *d_values, int n_bins, int max_iter, double *d_quantized,
                  double *d_centers, int32_t *d_info, void *d_workspace, size_t workspace_bytes,
                  void *stream);

/*
 * The reference's quantiser itself.  Replaces encode() (graphrole/roles/factor.py:29-49) with the SAME procedure
 * sklearn runs there: KMeans(n_clusters=k, random_state=1) on the flattened entries -- k-means++ seeding driven by
 * the caller's random numbers (drawn exactly as RandomState(1) hands them to sklearn: they do not depend on the
 * data), Lloyd iterations with sklearn's stopping rule (labels unchanged, or total squared centre shift <=
 * 1e-4 * var), empty-cluster relocation, every entry replaced by its cluster centre.  Centres agree with sklearn's
 * to ~1e-12 (sums are reduced in another order); the model selection of RolX then picks the reference's cell.
 * The seeding does not stream all m values per seed as sklearn's _kmeans_plusplus (:163-257) does: on the line a
 * candidate changes closest distances only in a contiguous range of the sorted values, and the sums the candidate
 * INDEX is drawn from (sklearn's cumulative sum in index order) are exact fixed-point integers (csrc/grx_kmeans.hip)
 * -- same seeds, O(m log k) instead of O(m k) work.  The candidates' potentials, which only feed an argmin, come from
 * fp64 sums over blocks of sorted values (first minimum, potentials within 1e-12 count as tied: sklearn's own are BLAS
 * sums in another order).
 *   d_values      fp64[m] in the order the reference flattens the matrix (row-major n x r for the node-role
 *                 factor: grx_transpose from the feature-major device layout)
 *   first_seed    RandomState(1).choice(m, p = uniform)            (sklearn _kmeans_plusplus, first centre)
 *   h_uniform     (k - 1) x n_trials doubles, n_trials = 2 + int(log(k)): RandomState.uniform(size=n_trials) per seed
 *   max_iter, rel_tol   sklearn defaults 300, 1e-4
 *   d_centers     fp64[k] in seed order;  d_info int32[4] = {Lloyd iterations (n_iter_), non-empty clusters,
 *                 distinct output values, seeding faults (0 unless an internal consistency check failed: bit 0 the
 *                 block sums after an update differ from potential - gain (exact gains, GRX_KMEANS_GAIN_PASS=1), bit 1
 *                 values beyond 1e144, bit 2 a cumulative-sum search left its block, bit 3 the potential after an
 *                 update is further than 1e-9 from potential - gain (fp64 gains, the default), bit 4 a workgroup of
 *                 the pick waited in vain for the others of its launch)}.
 *                 k <= 8192 (GRX_ERR_UNSUPPORTED above), k <= m (GRX_ERR_INVALID).
 * Environment (read once; for tests/test_gpu_encode.py, which runs every mode on the same inputs and compares bits):
 * GRX_KMEANS_FULL_RANGE=1 every range [0, m); GRX_KMEANS_GAIN_PASS=1 gains by an integer pass over each range;
 * GRX_KMEANS_SLOW_PICK=1 range positions by searches over all values; GRX_KMEANS_MERGE=0 the update always in its own
 * kernel; GRX_KMEANS_SMALL=0 no one-workgroup seeding of m <= 4096; GRX_KMEANS_LOSE_A_SUM=<seed> (test of the bounded
 * waits) one workgroup of that seed's launch withholds its sum: the run ends within a second with fault bit 4.
 * grx_transpose: out[c * ld_out + r] = in[r * ld_in + c].
 */
size_t grx_kmeans1d_workspace_bytes(int64_t m, int k);
int grx_kmeans1d(int64_t m, const double *d_values, int k, int64_t first_seed, const double *h_uniform, int n_trials,
                 int max_iter, double rel_tol, double *d_quantized, double *d_centers, int32_t *d_info,
                 void *d_workspace, size_t workspace_bytes, void *stream);
int grx_transpose(int64_t rows, int64_t cols, const double *d_in, int64_t ld_in, double *d_out, int64_t ld_out,
                  void *stream);


/* ------------------------------------------------------------------ RolX roles ---------- */
/*
 * The two row passes over the fitted node-role factor.  d_G: fp64 n x r row-major (the layout of the reference's
 * node_role_factor.values), any r >= 1 (the limit of the NMF kernels, GRX_MAX_ROLES, does not apply: a caller may
 * assign a wider frame).
 *   grx_role_argmax    replaces RoleExtractor.roles (graphrole/roles/extract.py:38-47, DataFrame.idxmax(axis=1)):
 *                      d_first_max int32[n] = column of the FIRST maximum of every row (quantised factors are full
 *                      of exact ties), NaN entries skipped, -1 for a row of NaNs only.
 *   grx_row_normalise  replaces RoleExtractor.role_percentage (:49-57, apply(lambda row: row / row.sum(), axis=1)):
 *                      d_share fp64 n x r = every row divided by its sum, the sum evaluated in the order
 *                      Series.sum() adds r doubles (numpy pairwise_sum: left to right below 8 values, eight strided
 *                      accumulators from 8 on; NaN counts as 0) -- bit-equal to the reference; 0 / 0 = NaN as there.
 */
int grx_role_argmax(int64_t n, int r, const double *d_G, int32_t *d_first_max, void *stream);
int grx_row_normalise(int64_t n, int r, const double *d_G, double *d_share, void *stream);

/* ------------------------------------------------------------------ sense making -------- */
/*
 * Node measures of RolX sense making (Henderson et al., KDD 2012: E >= 0 with G E ~ M, M = node x measure table).
 * The reference's RoleExtractor.explain() is a stub (graphrole/roles/extract.py); each measure restates networkx 3.4.2.
 * Graph arguments are the CSR convention above; every vector is in the caller's row order.
 *
 * grx_pagerank restates networkx.pagerank(G, alpha, weight='weight', tol, max_iter) (pagerank_alg.py,
 *   _pagerank_scipy): x0 = 1/N, x' = alpha (x A + sum(x[dangling]) / N) + (1 - alpha) / N with A = W scaled by the
 *   inverse out-weight, dangling = out-weight 0; stop at the first iteration with sum |x' - x| < N tol.
 *   d_in_*: the IN-adjacency, pulled (undirected: the CSR itself; directed: the transposed CSR), d_in_w NULL = 1.
 *   d_out_weight: fp64[n] out-weight row sums of the same graph (an undirected self-loop once).
 * grx_eigenvector_centrality restates networkx.eigenvector_centrality(G, max_iter, tol, weight='weight')
 *   (eigenvector.py): x0 = 1/N, x' = (A^T + I) x normalised to unit L2 norm, same stopping rule.
 * Both: rows longer than GRX_HUB_FACTOR * lanes_per_row (4, 8, 16 or 32 lanes per row) must be listed in
 *   d_hub_rows (int32 row ids) and are summed by a workgroup each.  The iterations are enqueued in batches; a device
 *   `done` word makes the launches after convergence return at once, the host reads it back once per batch.
 *   *h_iterations = iterations run.  Returns GRX_ERR_NOT_CONVERGED (d_x untouched) when max_iter iterations did not
 *   converge.  Deterministic: no floating-point atomics, partial sums reduced in a fixed order.
 *   d_workspace: grx_*_workspace_bytes(n) bytes.
 */
size_t grx_pagerank_workspace_bytes(int64_t n);
int grx_pagerank(int64_t n, const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                 const double *d_out_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                 double alpha, double tol, int max_iter, double *d_x, int *h_iterations, void *d_workspace,
                 size_t workspace_bytes, void *stream);
size_t grx_eigenvector_centrality_workspace_bytes(int64_t n);
int grx_eigenvector_centrality(int64_t n, const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                               const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, double tol,
                               int max_iter, double *d_x, int *h_iterations, void *d_workspace, size_t workspace_bytes,
                               void *stream);
/*
 * grx_local_structure_measures restates, for an undirected graph without parallel edges, networkx.clustering(G)
 *   (cluster.py, _triangles_and_degree_iter: 0 if T = 0 else 2T / (d' (d' - 1))) and networkx.effective_size(G)
 *   (structuralholes.py, Borgatti: d' - 2t / d', t = T + number of neighbours with a self-loop; NaN for an isolated
 *   node).  d' = degree without the self-loop, T = per-node triangle counts of grx_triangle_counts.  The same IEEE
 *   operations in the same order: bit-equal.  One divergence: a node whose only neighbour is itself gets NaN
 *   (networkx raises ZeroDivisionError).  d_loop_scratch: uint8[n] when the graph has self-loops, NULL when it has
 *   none (then d_col is not read).
 */
int grx_local_structure_measures(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const uint64_t *d_T,
                                 uint8_t *d_loop_scratch, double *d_clustering, double *d_effective_size, void *stream);
/*
 * grx_host_nnls: HOST.  Column by column, min_{e >= 0} || G e - m_j ||^2 from the normal equations (h_GtG r x r,
 *   h_GtM r x m, both row-major, from one grx_gram pass over [G | M]); Lawson-Hanson active set with a Cholesky
 *   factorisation of the passive block (scipy.optimize.nnls solves the same problem from G and M themselves).
 *   r <= GRX_MAX_ROLES, any m.  h_MtM_diag (optional, m values ||m_j||^2) scales the optimality tolerance.  Roles that
 *   are all zero, or linearly dependent on roles already passive, stay at 0.  h_E: r x m row-major.
 */
int grx_host_nnls(int r, int m, const double *h_GtG, const double *h_GtM, const double *h_MtM_diag, double *h_E);
/*
 * grx_betweenness restates networkx.betweenness_centrality(G, k, normalized, weight=None, endpoints, seed) (betweenness.py,
 *   unweighted: _single_source_shortest_path_basic, _accumulate_basic / _accumulate_endpoints, _rescale) for the
 *   sources d_sources[0 .. n_sources) (int32 row ids, distinct or not) in that order -- networkx's `for s in nodes`.
 *   Per source: a BFS counts the shortest paths sigma (pulled over the in-adjacency, level by level), then deepest
 *   level first delta(v) = sum over successors w one level deeper of sigma(v) * coeff(w), coeff(w) = (1 + delta(w)) /
 *   sigma(w) (pulled over the out-adjacency); bc[w] += delta(w) for every reached w != s (endpoints: += delta(w) + 1,
 *   and bc[s] += reached - 1).  Finally bc *= scale (the caller computes _rescale's factor, 1 for none).
 *   d_row_ptr / d_col: the out-adjacency; d_in_row_ptr / d_in_col: the in-adjacency (transposed CSR) of a directed
 *   graph, NULL for an undirected one.  Weights are not read; self-loops never lie on a shortest path.  Rows longer
 *   than GRX_HUB_FACTOR * lanes_per_row (resp. in_lanes_per_row) must be listed in d_hub_rows (resp. d_in_hub_rows).
 *   batch: sources per batch B, a multiple of 64 up to 256; 0 = the library's choice: the widest B whose state fits
 *   4 GiB, but never below 64 (so above ~3.35 M nodes the state is 20 n 64 bytes, more than 4 GiB), and no wider than
 *   the source list rounded up to 64.  State: 20 n B bytes (level int32, sigma and delta fp64 per node and source).
 *   Bound: sigma must stay below 2^53 (path counts; networkx's floats round beyond that too).
 *   Deterministic and the same bits for every B: bc[v] adds its sources' terms one source after another in the order
 *   of d_sources, no floating-point atomics.  Against networkx only the order of the additions inside one delta(v)
 *   differs (networkx: reverse BFS order of the successors; here: column order), so results agree to 1e-12 relative.
 *   d_bc: fp64[n], overwritten.  d_workspace: grx_betweenness_workspace_bytes(n, batch, n_sources) bytes.
 */
size_t grx_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources);
int grx_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                    int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                    const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                    const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch, double *d_bc,
                    void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_distance_sums: per-target BFS distance sums from many sources -- what networkx.closeness_centrality(G, u,
 *   distance=None, wf_improved) (closeness.py:107-137) and networkx.harmonic_centrality(G, nbunch, distance=None,
 *   sources) (harmonic.py:68-89) compute from.  For every node v and the sources s = d_sources[0 .. n_sources)
 *   (int32 row ids; a repeated id counts once per occurrence) along the arcs the caller lists:
 *     reach[v]    = number of sources s != v with a path s -> v                       (networkx: len(sp) - 1)
 *     dsum[v]     = sum of d(s, v) over those sources                                 (networkx: totsp)
 *     harmonic[v] = sum of fl(1 / d(s, v)) over those sources, correctly rounded      (networkx: sum of 1 / d)
 *   The BFS PULLS over d_row_ptr / d_col: next(v) collects the frontier of the nodes listed in v's row.  So pass the
 *   in-adjacency (transposed CSR) to walk the out-arcs from each source -- closeness of every node and harmonic
 *   centrality -- and the out-adjacency to walk the reversed arcs from one source (closeness(G, u): networkx walks
 *   G.reverse()); an undirected graph's CSR is both.  Weights are not read; self-loops and parallel arcs never change
 *   a distance.  Rows longer than GRX_HUB_FACTOR * lanes_per_row must be listed in d_hub_rows.
 *   Method: a bitset multi-source BFS (Then et al., VLDB 2014), S = 64 words sources per batch; per node three masks
 *   of `words` uint64 (visited and two frontiers: state 24 n words bytes).  words: 1, 2, 4, 8 or 16; 0 = the
 *   library's choice: the narrowest power of two that holds the source list, at most the widest one up to 16 whose
 *   state fits 4 GiB, and at least 1.
 *   Exact: reach and dsum are integer sums (dsum <= n^2 < 2^62); harmonic is summed in a 128-bit fixed-point integer
 *   (fl(1 / d) is a whole multiple of 2^-84 for d < 2^31) and rounded once to nearest-even, so every output has the
 *   same bits for every `words`, source order and run.  networkx's closeness follows bit for bit from reach and dsum
 *   (its own three IEEE operations); networkx's harmonic adds the same terms one by one, so it agrees to 1e-12.
 *   d_reach, d_dsum: int64[n], d_harmonic: fp64[n], all overwritten.  n < 2^31.
 *   d_workspace: grx_distance_sums_workspace_bytes(n, words, n_sources) bytes.
 */
size_t grx_distance_sums_workspace_bytes(int64_t n, int words, int64_t n_sources);
int grx_distance_sums(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                      int64_t n_hub_rows, int lanes_per_row, const int32_t *d_sources, int64_t n_sources, int words,
                      int64_t *d_reach, int64_t *d_dsum, double *d_harmonic, void *d_workspace,
                      size_t workspace_bytes, void *stream);

/*
 * grx_eccentricity: the eccentricity of many BFS sources at once, and bounds on the eccentricity of every node -- what
 *   networkx.eccentricity(G, v) (distance_measures.py) computes one BFS per node.  The graph, the source list, `words`
 *   and the pulling direction are those of grx_distance_sums (same bitset BFS, S = 64 words sources per batch; state
 *   24 n words bytes).  Per batch, pass A runs one BFS:
 *     source_ecc[b] = the largest d(s_b, v) over the nodes v that s_b reaches; 0 when it reaches nothing (or when
 *                     s_b lies outside [0, n): such an id is never written through)
 *     reach[v]     += number of the batch's sources s != v with a path s -> v (a repeated id counts per occurrence)
 *     lower[v]      = max(lower[v], largest d(s, v) over those sources): the per-target maximum distance
 *   With d_upper non-NULL pass B replays the batch's BFS, source_ecc now known, and tightens the eccentricity bounds of
 *   Takes and Kosters ("Computing the eccentricity distribution of large graphs", 2013) for every v and every source s
 *   of the batch with a path to v at distance d >= 0 (d = 0: v = s):
 *     upper[v] = min(upper[v], d + source_ecc[s]),   lower[v] = max(lower[v], source_ecc[s] - d)
 *   so that lower[s] = upper[s] = source_ecc[s] at every source.  Pass B is VALID ONLY ON A SYMMETRIC CSR (an undirected
 *   graph, d(s, v) = d(v, s)) whose sources reach every node; then lower <= ecc <= upper elementwise.  On a directed
 *   graph pass NULL for d_upper: source_ecc is right for any CSR, lower is then the per-target maximum only.
 *   accumulate = 0: the call first sets reach = 0, lower = 0 and upper = INT32_MAX; 1: it continues from the caller's
 *   arrays (bounds carried across calls).  d_source_ecc: int32[n_sources], overwritten; d_reach: int64[n]; d_lower,
 *   d_upper: int32[n].  Integer arithmetic only; every output is the same for every `words`, source order and run.
 *   n < 2^31.  d_workspace: grx_eccentricity_workspace_bytes(n, words, n_sources) bytes.
 */
size_t grx_eccentricity_workspace_bytes(int64_t n, int words, int64_t n_sources);
int grx_eccentricity(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                     int64_t n_hub_rows, int lanes_per_row, const int32_t *d_sources, int64_t n_sources, int words,
                     int32_t *d_source_ecc, int64_t *d_reach, int32_t *d_lower, int32_t *d_upper, int accumulate,
                     void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_weighted_distances: shortest-path distances by arc weight from many sources -- every source's
 *   networkx.single_source_dijkstra_path_length(G, s, weight) -- and what closeness_centrality(G, distance=...),
 *   harmonic_centrality(G, distance=...) and eccentricity(G, weight=...) compute from them.  The graph, the hub list,
 *   the source list (int32 row ids, a repeated id counts once per occurrence, an id outside [0, n) is never written
 *   through and reaches nothing) and the pulling direction are those of grx_distance_sums: pass the in-adjacency with
 *   its weights to walk the out-arcs from each source.  d_w: fp64 per entry of d_col, the weight of that arc; NULL =
 *   every weight is 1.  CONTRACT: every weight finite and >= 0 (the caller checks; parallel arcs are fine here -- the
 *   lightest one wins -- and a self-loop never shortens a path).
 *   For every node v and the sources s_0 .. s_{n_sources-1}, in that order:
 *     reach[v]      = number of source occurrences s != v with a path s -> v
 *     dsum[v]       = their distances d(s, v), added one by one from 0.0 in the order of d_sources
 *     harmonic[v]   = fl(1 / d(s, v)) of those with d > 0, added likewise (networkx skips distance 0 as well)
 *     far[v]        = the largest of those distances, 0.0 if there is none
 *     source_ecc[b] = the largest finite d(s_b, v) over all v; 0.0 when s_b reaches nothing
 *     dist[b * ld_dist + v] = d(s_b, v), +inf without a path (d_dist may be NULL; otherwise ld_dist >= n)
 *   Method: a batched Bellman-Ford relaxation from +inf, S = `batch` sources at a time (16, 32 or 64; 0 = the library's
 *   choice: the widest whose state fits 4 GiB, never below 16, no wider than the source list rounded up), S lanes per
 *   node over fp64 state dist[v * S + b], Jacobi rounds over two buffers, a per-node stamp of the last round that
 *   lowered it so that a row is stored only while it moves, device-steered rounds (8 per read-back) until one lowers
 *   nothing; see the header of csrc/grx_sssp.hip.  State: 16 n S + 4 n bytes.  Work: every round gathers 8 S bytes
 *   per arc; the number of rounds per batch is (the most arcs on any lightest path from its sources) + 1.  More than n + 1 rounds (a weight
 *   outside the contract) return GRX_ERR_INVALID.
 *   Exact: with weights >= 0 the distance is the minimum over the paths of the left-to-right fp64 sum of the weights,
 *   which is what networkx's Dijkstra returns and the only fixed point of the relaxation: dist and source_ecc equal
 *   networkx bit for bit.  The sums run in source order with no floating-point atomics, so every output has the same
 *   bits for every `batch` and run; networkx adds the same terms in another order (closeness: its pop order;
 *   harmonic: a set's), so dsum is equal for integer weights and both agree to 1e-12 relative otherwise.
 *   d_reach: int64[n]; d_dsum, d_harmonic, d_far: fp64[n]; d_source_ecc: fp64[n_sources]; all overwritten.
 *   h_rounds: HOST int64 or NULL: the rounds run, summed over the batches (reading it needs no extra wait: the call
 *   waits for the stream once per 8 rounds anyway).  Returns GRX_ERR_INVALID before any HIP call for batch outside
 *   {0, 16, 32, 64}, n outside [1, 2^31), n_sources < 0, d_dist with ld_dist < n and a short workspace.
 *   d_workspace: grx_weighted_distances_workspace_bytes(n, batch, n_sources) bytes.
 */
size_t grx_weighted_distances_workspace_bytes(int64_t n, int batch, int64_t n_sources);
int grx_weighted_distances(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                           const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                           const int32_t *d_sources, int64_t n_sources, int batch,
                           int64_t *d_reach, double *d_dsum, double *d_harmonic, double *d_far,
                           double *d_source_ecc, double *d_dist, int64_t ld_dist, int64_t *h_rounds,
                           void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_weighted_betweenness restates networkx.betweenness_centrality(G, k, normalized, weight, endpoints, seed) for a
 *   weight attribute (betweenness.py: _single_source_dijkstra_path_basic, _accumulate_basic / _accumulate_endpoints,
 *   _rescale) for the sources d_sources[0 .. n_sources) (int32 row ids, distinct or not, an id outside [0, n) reaches
 *   nothing) in that order, without a priority queue.  Per batch of S sources: the relaxation of
 *   grx_weighted_distances gives networkx's Dijkstra distances D bit for bit; arc u -> v of weight w lies on a lightest
 *   path from a source iff D(v) is finite, fl(D(u) + w) == D(v) and D(u) < D(v) (networkx's own equality of fp64 sums;
 *   the strict inequality keeps the relation acyclic); a device-steered round loop gives every reached node its depth in
 *   that DAG and sigma = the sum of its predecessors' sigma once ALL of them are resolved (pulled over the in-adjacency);
 *   then deepest level first delta(v) = sum over the DAG successors x of sigma(v) * coeff(x), coeff(x) = (1 + delta(x))
 *   / sigma(x) (pulled over the out-adjacency); bc[w] += delta(w) for every reached w != s (endpoints: += delta(w) + 1,
 *   and bc[s] += reached - 1).  Finally bc *= scale (the caller computes _rescale's factor, 1 for none).
 *   d_row_ptr / d_col / d_w: the out-adjacency with its fp64 weights; d_in_row_ptr / d_in_col / d_in_w: the
 *   in-adjacency (transposed CSR) with its weights of a directed graph, d_in_row_ptr NULL for an undirected one (the out
 *   CSR then serves both passes).  d_w NULL = every weight is 1 (then d_in_w NULL as well).  CONTRACT: every weight
 *   finite and > 0 (the caller checks).  A zero weight would let networkx count paths through nodes it has already
 *   settled, so its own result depends on its heap order; here an arc whose weight is absorbed (fl(d + w) == d) or zero
 *   is not a shortest-path arc, and a node reached only through such arcs counts as not reached: stated divergences.
 *   Rows longer than GRX_HUB_FACTOR * lanes_per_row (resp. in_lanes_per_row) must be listed in d_hub_rows (resp.
 *   d_in_hub_rows).  batch: S = 16, 32 or 64; 0 = the library's choice: the widest whose state fits 4 GiB, never below
 *   16, no wider than the source list rounded up.  State: 28 n S + 4 n bytes (two distance buffers -- the second
 *   becomes delta once the relaxation has converged --, sigma, depth, the relaxation's stamps).
 *   Bound: sigma must stay below 2^53.  Deterministic and the same bits for every S and run: bc[v] adds its sources'
 *   terms one source after another in the order of d_sources, hub rows combine four partial sums in a fixed order for
 *   every S, no floating-point atomics.  Against networkx only the order of the additions inside one delta(v)
 *   differs, so results agree to 1e-12 relative and entries networkx has at exactly 0 are exactly 0.
 *   d_bc: fp64[n], overwritten.  h_rounds: HOST int64 or NULL: the relaxation rounds run, summed over the batches;
 *   h_levels: HOST int64 or NULL: the deepest DAG level of any batch (with unit weights: the BFS depth).  Returns
 *   GRX_ERR_INVALID before any HIP call for batch outside {0, 16, 32, 64}, n outside [1, 2^31), a bad source list, hub
 *   list or lanes_per_row, null pointers and a short workspace; and when the relaxation or the forward pass runs more
 *   than n + 1 rounds (weights outside the contract): an error, never a hang.
 *   d_workspace: grx_weighted_betweenness_workspace_bytes(n, batch, n_sources) bytes.
 */
size_t grx_weighted_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources);
int grx_weighted_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                             const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                             const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                             const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                             const int32_t *d_sources, int64_t n_sources, int endpoints, double scale, int batch,
                             double *d_bc, int64_t *h_rounds, int64_t *h_levels, void *d_workspace,
                             size_t workspace_bytes, void *stream);

/*
 * grx_edge_betweenness restates networkx.edge_betweenness_centrality(G, k, normalized, weight=None, seed) (betweenness.py:
 *   edge_betweenness_centrality, _single_source_shortest_path_basic, _accumulate_edges, _rescale_e) for the sources
 *   d_sources[0 .. n_sources) in that order: the forward and backward passes of grx_betweenness (same kernels, same
 *   arguments without `endpoints`) with coeff kept in an array of its own, so that sigma survives; then, per batch, the
 *   slot of every arc v -> w of a source's BFS DAG (level(w) == level(v) + 1) adds c = sigma(v) * coeff(w), networkx's
 *   own term of _accumulate_edges.  d_ebc: fp64, one value per arc of the out CSR (d_row_ptr / d_col), overwritten.
 *   Directed (d_in_row_ptr given): the slot of u -> v is the arc's sum times scale.  Undirected: networkx keeps one key
 *   per edge; for one source only one of its two arcs is a DAG arc, so the edge is (slot(u -> v) + slot(v -> u)) *
 *   scale, and BOTH slots of the edge hold that value at the end (the mirror slot is found by binary search in the
 *   sorted row; the rows must be sorted and the CSR symmetric).  Self-loop slots are exactly 0.0.  scale: the caller
 *   computes _rescale_e's factor, 1 for none (networkx 3.4.2 does not pass k to _rescale_e: no n / k for sampled
 *   sources).  batch: as grx_betweenness, with 28 n B bytes of state (level, sigma, delta, coeff).
 *   ORDER of the additions into a slot: the source list is cut into aligned groups of 16 consecutive sources; a group's
 *   16 terms (+0.0 where the arc is no DAG arc of the source or the list has ended) are summed by the fixed pairwise
 *   tree (((t0 + t1) + (t2 + t3)) + ...), and the group sums are added one after another in source order onto the slot.
 *   That depends on a source's position in d_sources alone: the same bits for every B, launch shape and run; no
 *   floating-point atomics (one wavefront owns a slot).  Against networkx only the order in which a slot adds its
 *   sources and the order inside one delta(v) differ: 1e-12 relative; values networkx has at exactly 0 are exactly 0.
 *   d_workspace: grx_edge_betweenness_workspace_bytes(n, batch, n_sources) bytes.  Errors as grx_betweenness.
 */
size_t grx_edge_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources);
int grx_edge_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                         int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                         const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                         const int32_t *d_sources, int64_t n_sources, double scale, int batch, double *d_ebc,
                         void *d_workspace, size_t workspace_bytes, void *stream);
/*
 * grx_weighted_edge_betweenness restates networkx.edge_betweenness_centrality(G, k, normalized, weight, seed) for a
 *   weight attribute (betweenness.py: edge_betweenness_centrality, _single_source_dijkstra_path_basic,
 *   _accumulate_edges, _rescale_e): the relaxation, forward and backward passes of grx_weighted_betweenness (same
 *   kernels, same arguments without `endpoints`, same contract on the weights and the same stated divergences) with
 *   coeff kept in an array of its own; then, per batch of S sources, the slot of every arc u -> v of a source's
 *   shortest-path DAG (fl(D(u) + w) == D(v) and D(u) < D(v), u resolved, v deeper) adds sigma(u) * coeff(v).
 *   d_ebc, directed / undirected slots, self-loops, scale, the ORDER of the additions and the tolerance against
 *   networkx: as grx_edge_betweenness -- the same bits for S = 16, 32 and 64.  State: 36 n S + 4 n bytes.
 *   h_rounds / h_levels: as grx_weighted_betweenness.
 *   d_workspace: grx_weighted_edge_betweenness_workspace_bytes(n, batch, n_sources) bytes.
 */
size_t grx_weighted_edge_betweenness_workspace_bytes(int64_t n, int batch, int64_t n_sources);
int grx_weighted_edge_betweenness(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                                  const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                                  const int64_t *d_in_row_ptr, const int32_t *d_in_col, const double *d_in_w,
                                  const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row,
                                  const int32_t *d_sources, int64_t n_sources, double scale, int batch, double *d_ebc,
                                  int64_t *h_rounds, int64_t *h_levels, void *d_workspace, size_t workspace_bytes,
                                  void *stream);

/*
 * grx_biconnected: for every node of an undirected graph the number of biconnected components it belongs to -- what
 *   Counter(v for c in networkx.biconnected_components(G) for v in c) counts, and more than one exactly for the nodes
 *   of networkx.articulation_points(G) (networkx/algorithms/components/biconnected.py: biconnected_components,
 *   articulation_points; both a depth-first search) -- together with a spanning forest and a component label per tree
 *   edge from which the components themselves follow.
 *   d_row_ptr / d_col: the CSR of the graph's distinct arcs, symmetric (every edge from both ends), rows in any order;
 *   self-loop entries are skipped, weights are not read.  Rows longer than GRX_HUB_FACTOR * lanes_per_row must be
 *   listed in d_hub_rows.
 *   Method: Tarjan-Vishkin (SIAM J. Comput. 1985) on a BFS spanning forest, level-synchronous: connected components
 *   by lock-free union-find (roots = the smallest id of each component), a BFS from every root at once, subtree sizes,
 *   preorder numbers, low / high over the non-tree edges, then a second union-find over the tree edges; see the header
 *   of csrc/grx_biconnected.hip.  O(n + m) work per sweep and O(D) launches for BFS depth D; the level count is read
 *   back once per 8 levels.  A deep graph (a path) is bound by launch latency.
 *   d_count:  int64[n], overwritten; 0 for an isolated node and for a node whose only arc is a self-loop.
 *   d_parent: int32[n] or NULL: the BFS forest, parent[v] = the smallest id among v's neighbours one level nearer to
 *             the root, -1 for a root (the smallest id of its connected component).  The same in every run.
 *   d_label:  int32[n] or NULL: label[c] names the biconnected component of the tree edge (parent[c], c) -- the
 *             smallest c among the component's tree edges -- and is -1 for a root.  Component r is the union of
 *             {c, parent[c]} over the c with label[c] = r.
 *   n_components: HOST int64 or NULL: the number of biconnected components (reading it waits for the stream).
 *   Exact (integers only; integer atomics whose results do not depend on their order): every output has the same
 *   bits in every run.  n < 2^31.  d_workspace: grx_biconnected_workspace_bytes(n) bytes (about 40 n).
 */
size_t grx_biconnected_workspace_bytes(int64_t n);
int grx_biconnected(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                    int64_t n_hub_rows, int lanes_per_row, int64_t *d_count, int32_t *d_parent, int32_t *d_label,
                    int64_t *n_components, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_core_numbers: the core number of every node -- networkx.core_number(G) (networkx/algorithms/core.py) -- and,
 *   for an undirected graph, its onion layer -- networkx.onion_layers(G): the round in which the node is peeled -- by
 *   synchronous peeling: k = max(k, min degree over the alive nodes); every alive node of degree <= k (degrees as at
 *   the start of the round) gets core = k and onion = the round's number (from 1) and leaves; the degree of every
 *   node at the other end of one of its arcs drops by one.
 *   d_row_ptr / d_col: the CSR of the graph's distinct arcs, rows in any order.  All d_in_* NULL / 0: an undirected
 *   graph, the CSR symmetric (every edge from both ends).  Otherwise a directed graph: the first CSR holds the
 *   out-arcs, d_in_row_ptr / d_in_col the in-arcs (its transpose); degree = in + out, a leaving node decrements along
 *   both, so a reciprocal pair counts twice (networkx's all_neighbors); d_onion is then the peeling round as well,
 *   which networkx does not define.  PRECONDITION: no self-loop entry in either CSR (networkx raises
 *   NetworkXNotImplemented for such a graph; the caller refuses it).  Weights are not read.  Rows longer than
 *   GRX_HUB_FACTOR * lanes_per_row (in_lanes_per_row) must be listed in d_hub_rows (d_in_hub_rows).
 *   Method: see the headers of csrc/grx_kcore.hip and csrc/grx_peel.h (the peeling core it shares with
 *   grx_truss_numbers).  The next round's nodes are collected in a list by the decrement
 *   that takes a node's degree from above k to k or below; all n nodes are swept (twice) only when k jumps.  Cost: 2
 *   sweeps per distinct core value, every arc visited once from each end over the whole run, and every alive hub row
 *   read once per round (a hub pulls its decrement instead of taking one atomic per leaving neighbour).  16 rounds
 *   are enqueued per read-back of (done, round).
 *   d_core:  int64[n], overwritten.   d_onion: int64[n] or NULL.
 *   n_rounds: HOST int64 or NULL: the number of rounds run = the largest onion layer.
 *   Exact (integers only; the outputs do not depend on the order of the atomics): the same bits in every run.
 *   n < 2^31.  d_workspace: grx_core_numbers_workspace_bytes(n) bytes (about 16 n).  The call waits for the stream.
 */
size_t grx_core_numbers_workspace_bytes(int64_t n);
int grx_core_numbers(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                     int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                     const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, int64_t *d_core,
                     int64_t *d_onion, int64_t *n_rounds, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_structural_holes: Burt's structural-hole measures of every node -- networkx.constraint(G, weight=...),
 *   networkx.local_constraint of every arc and the weighted / directed form of networkx.effective_size
 *   (networkx/algorithms/structuralholes.py).  With z(u, v) networkx's mutual_weight w(u -> v) + w(v -> u),
 *     S(u) = sum_x z(u, x),  X(u) = max_x z(u, x),  P(u, v) = z(u, v) / S(u),  M(v, w) = z(v, w) / X(v)   (0 / 0 = 0)
 *     local(u, v)       = (P(u, v) + sum_w P(u, w) P(w, v))^2        constraint(u) = sum_v local(u, v)
 *     effective_size(u) = sum_v (1 - sum_w P(u, w) M(v, w))
 *   v over the entries of row u (u itself when it has a self-loop), w over the common entries of rows u and v.
 *   d_row_ptr / d_col: a CSR that is SYMMETRIC in structure (entry (u, v) iff entry (v, u)); columns ascending and
 *   distinct inside a row; a diagonal entry is allowed.  Rows in any order.  Rows longer than GRX_HUB_FACTOR *
 *   lanes_per_row (4, 8, 16 or 32) must be listed in d_hub_rows.
 *   d_z: fp64[nnz], the mutual weights: symmetric (the value at arc (u, v) equals the value at (v, u)), finite and
 *   >= 0; NULL = every z is 1 (P and M then come from the row lengths alone).  A common factor of all z cancels in P
 *   and M: an undirected graph may pass its edge weights w for z = 2 w.
 *   d_out_row_ptr: int64[n+1], the row pointers of the graph's own out-adjacency in the same row order, or NULL = those
 *   of the CSR itself.  A node whose row is empty THERE gets NaN in both node outputs (networkx: len(G[v]) == 0; a
 *   directed node with in-arcs only).  Only the row lengths are read.
 *   d_constraint, d_effective_size: fp64[n] or NULL.  d_local: fp64[nnz] or NULL, local(u, v) at arc (u, v).  At least
 *   one must be given.  d_effective_size always holds the sum above; for an undirected graph without weights networkx
 *   uses the ego-graph formula n - 2t/n instead (grx_local_structure_measures), which is the caller's choice.
 *   Method: see the header of csrc/grx_structural_holes.hip: row statistics, then one lane group per ARC that walks
 *   the shorter of the two rows and binary-searches the longer one, then a per-row sum of the arc terms.  Bound: the
 *   sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers plus two 8-byte gathers per
 *   common neighbour.  Every quotient and product is its own IEEE operation; sums are lane-strided with a fixed
 *   butterfly.  No floating-point atomics: every output has the same bits in every run.
 *   n < 2^31.  d_workspace: grx_structural_holes_workspace_bytes(n, nnz) bytes (16 n + 20 nnz), nnz = row_ptr[n]; the
 *   call reads row_ptr[n] back to check it and so waits for the stream once, before its first launch.
 */
size_t grx_structural_holes_workspace_bytes(int64_t n, int64_t nnz);
int grx_structural_holes(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_z,
                         const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                         const int64_t *d_out_row_ptr,
                         double *d_constraint, double *d_effective_size, double *d_local,
                         void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_clustering: the clustering coefficient of every node in its weighted and its directed forms --
 *   networkx.clustering(G, weight=...) of an undirected graph with weights (Onnela: the geometric mean of the three
 *   normalised weights of each triangle), of a directed graph (Fagiolo) and of a directed graph with weights
 *   (networkx/algorithms/cluster.py).  With a value s per arc of the CSR
 *     undirected  s(u, v) = cbrt(w(u, v) / max_weight)
 *     directed    s(u, v) = cbrt(w(u -> v) / max_weight) + cbrt(w(v -> u) / max_weight), an absent direction adds 0
 *     t(u) = sum_v s(u, v) * sum_w s(u, w) * s(v, w)          clustering(u) = t == 0 ? 0 : t / denominator(u)
 *   v over the entries of row u other than u, w over the common entries of rows u and v other than u and v, and
 *     undirected  denominator = d (d - 1),               d = the entries of row u other than u
 *     directed    denominator = 2 (dt (dt - 1) - 2 db),  dt = the directions present at those entries, db = dt - d
 *   (undirected: t is twice networkx's weighted_triangles; directed: its directed_triangles).
 *   d_row_ptr / d_col: a CSR that is SYMMETRIC in structure (entry (u, v) iff entry (v, u)): row u lists every
 *   neighbour of u in EITHER direction; columns ascending and distinct inside a row; a diagonal entry is allowed and
 *   counts neither as a neighbour nor in a triangle.  Rows in any order.  Rows longer than GRX_HUB_FACTOR *
 *   lanes_per_row (4, 8, 16 or 32) must be listed in d_hub_rows.
 *   d_fwd: fp64[nnz], at arc (u, v) the weight of u -> v; d_bwd: fp64[nnz], at arc (u, v) the weight of v -> u (so
 *   d_bwd at (u, v) equals d_fwd at (v, u)).  A NEGATIVE value marks a direction that is absent; at least one of the
 *   two is present at every arc; a present weight is finite and in [0, max_weight].  A weight of 0 is a present
 *   direction: it counts in dt and d and contributes 0 to t.
 *   d_bwd == NULL: an undirected graph, d_fwd symmetric and >= 0 everywhere.
 *   d_fwd == NULL (d_bwd must be NULL too): an undirected graph without weights; every s is 1, no value array is read
 *   and max_weight is ignored: the result has the bits of grx_local_structure_measures' clustering.  A directed graph
 *   without weights passes 1 for a present direction and max_weight = 1.
 *   max_weight: networkx's max over every edge, self-loops included; finite and > 0 whenever d_fwd is given.  A
 *   quotient w / max_weight that equals 1 has the cube root 1 without a call of cbrt: constant weights give the bits
 *   of the form without weights, and there every quantity is an integer, so the result is networkx's bit for bit.
 *   d_clustering: fp64[n], overwritten.  d_triangles: fp64[n] or NULL, t(u).
 *   Method: see the header of csrc/grx_clustering.hip: s and the denominator per row, then one lane group per ARC that
 *   walks the shorter of the two rows and binary-searches the longer one, then a per-row sum of the arc terms.  Bound:
 *   the sum over arcs of min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers plus one 8-byte gather per
 *   common neighbour; one cbrt per arc and direction, none inside the intersection.  Every quotient and product is its
 *   own IEEE operation; sums are lane-strided with a fixed butterfly.  No floating-point atomics: every output has
 *   the same bits in every run.
 *   n < 2^31.  d_workspace: grx_clustering_workspace_bytes(n, nnz) bytes (8 n + 20 nnz), nnz = row_ptr[n]; the call
 *   reads row_ptr[n] back to check it and so waits for the stream once, before its first launch.
 */
size_t grx_clustering_workspace_bytes(int64_t n, int64_t nnz);
int grx_clustering(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_fwd, const double *d_bwd,
                   double max_weight, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                   double *d_clustering, double *d_triangles, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_square_clustering: the square clustering coefficient of every node -- networkx.square_clustering(G)
 *   (networkx/algorithms/cluster.py; Lind et al. 2005, Zhang et al. 2008), the probability that two neighbours of a
 *   node share a common neighbour other than that node.  With N = the entries of row v (v itself among them when the
 *   row has a diagonal entry), d = |N| and k_u = the length of row u
 *     K1   = sum_{u in N} k_u
 *     c(x) = |{u in N : x in row u}|  for x != v           (row v of A^2, set semantics)
 *     Q    = sum_{x != v} c(x) (c(x) - 1) / 2              (networkx's numerator: the 4-cycles through v)
 *     S    = sum_{x in N, x != v} c(x),   L = |{x in N, x != v : row x has a diagonal entry}|
 *     potential = (d - 1) (K1 - d) - (S - L + (d - 1) [row v has a diagonal entry]) - Q
 *     square_clustering(v) = potential > 0 ? (double)Q / (double)potential : (double)Q
 *   which is networkx's sum over the pairs of neighbours, collapsed; every quantity is an integer until the division.
 *   networkx divides only when potential > 0 and otherwise leaves Q: 0 without self-loops; with them Q > 0 can occur.
 *   d_row_ptr / d_col: the CSR of the DISTINCT arcs of an undirected graph: SYMMETRIC (entry (u, v) iff entry (v, u));
 *   columns ascending and distinct inside a row; a diagonal entry is allowed and means a self-loop.  Rows in any order;
 *   no weights are read.  Rows longer than GRX_HUB_FACTOR * lanes_per_row (4, 8, 16 or 32) must be listed in d_hub_rows.
 *   d_square_clustering: fp64[n], overwritten.  d_squares: int64[n] or NULL, Q.  d_potential: int64[n] or NULL.
 *   n < 2^31.  While Q and potential are below 2^53 the quotient is Python's int / int: networkx's value bit for bit.
 *   Method: see the header of csrc/grx_square_clustering.hip: K1 and the self-loop flag per row, then one workgroup per
 *   row that counts c(x) over the row's K1 wedges v -> u -> x -- in an open-addressing table in LDS sized from K1
 *   (rows with K1 <= 3 072; LDS compare-and-swap and add) or in dense int32[n] counters of the workspace that a second
 *   walk over the wedges cleans (the rows above) -- and forms Q, S, L and the quotient.  Bound: 4 sum_u k_u^2 bytes of
 *   gathered column ids and one atomic per wedge.  Integer atomics only, whose combined result does not depend on
 *   their order: every output has the same bits in every run and for every lanes_per_row.
 *   d_workspace: grx_square_clustering_workspace_bytes(n) bytes = 8 n + 128 * 4 n (K1 and flag per row; 128 sets of dense
 *   counters, one per workgroup of the dense launch), each array rounded up to 256 bytes.  The call does not wait for
 *   the stream.
 */
size_t grx_square_clustering_workspace_bytes(int64_t n);
int grx_square_clustering(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                          int64_t n_hub_rows, int lanes_per_row, double *d_square_clustering, int64_t *d_squares,
                          int64_t *d_potential, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_truss_numbers: the truss number of every edge -- the largest k such that the edge belongs to
 *   networkx.k_truss(G, k) (networkx/algorithms/core.py; Cohen 2008), the maximal subgraph in which every edge lies in
 *   at least k - 2 triangles of that subgraph; at least 2 -- and of every node -- the largest truss number of an edge
 *   at it, 0 for a node without an edge (networkx drops isolated nodes from every truss) -- by one level-synchronous
 *   peeling of the edges (PKT: Kabir and Madduri 2017): sup(e) = the triangles through e; k = 2; the alive edges with
 *   sup <= k - 2 (supports as at the start of the round) get t = k and leave, and every triangle one of them closes
 *   with two edges that have not left in an earlier round is taken away exactly once: the support of each of its
 *   edges that stays drops by one; when no alive edge has sup <= k - 2, k = 2 + the least support of an alive edge.
 *   d_row_ptr / d_col: the CSR of the distinct arcs of an undirected graph: SYMMETRIC (entry (u, v) iff entry (v, u)),
 *   columns ascending and distinct inside a row.  Rows in any order; no weights are read.  PRECONDITION: no self-loop
 *   entry (networkx raises NetworkXNotImplemented for such a graph; the caller refuses it).  Rows longer than
 *   GRX_HUB_FACTOR * lanes_per_row (4, 8, 16 or 32) must be listed in d_hub_rows (the node column's launch shape; the
 *   intersections have no hub path: one group of lanes_per_row lanes per edge whatever the rows' lengths).
 *   d_arc_truss: int32[nnz], overwritten: t of the edge at BOTH of its arcs.
 *   d_node_truss: int64[n] or NULL.
 *   n_rounds: HOST int64 or NULL: the number of rounds run.  n_levels: HOST int64 or NULL: the distinct k assigned.
 *   Method: see the headers of csrc/grx_truss.hip and csrc/grx_peel.h (the peeling core it shares with
 *   grx_core_numbers).  The supports are one row intersection per edge (the per-arc kernel
 *   of csrc/grx_rowjoin.h at the arcs with row < column; the position of every arc's reverse by one binary search
 *   beside it); the next round's edges are collected in a list by the decrement that takes an edge's support from
 *   above k - 2 to k - 2; all arcs are swept (twice) only when k jumps.  Cost: 2 intersections per edge over the whole
 *   call, each min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers; in the peel two more 4-byte gathers
 *   per common neighbour and at most 3 integer atomic decrements per triangle; 2 sweeps of at most 8 nnz bytes per
 *   distinct k; 4 launches per round, 16 rounds enqueued per read-back of the control words.
 *   Exact (integers only; the outputs do not depend on the order of the atomics): the same bits in every run, for
 *   every lanes_per_row and for every relabelling of the rows.
 *   n < 2^31 and nnz = row_ptr[n] < 2^31 (per-arc positions are int32), nnz even.  d_workspace:
 *   grx_truss_numbers_workspace_bytes(n, nnz) bytes (24 nnz: six int32 per arc, each array rounded up to 256 bytes,
 *   + 256).  n == 0 or nnz == 0: GRX_OK with nothing launched but the zeroing of d_node_truss.  Otherwise the call
 *   reads row_ptr[n] back to check it and waits for the stream at every read-back of the round loop; the node
 *   column is enqueued behind the last one and not waited for.
 */
size_t grx_truss_numbers_workspace_bytes(int64_t n, int64_t nnz);
int grx_truss_numbers(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                      int64_t n_hub_rows, int lanes_per_row, int32_t *d_arc_truss, int64_t *d_node_truss,
                      int64_t *n_rounds, int64_t *n_levels, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_graphlet_orbits: the graphlet degree vector of every node (Przulj 2007): for each of the 15 automorphism orbits
 *   of the connected graphs on 2, 3 and 4 nodes, the number of INDUCED subgraphs that touch the node at that orbit.
 *     0 edge | 1, 2 path on 3: end, middle | 3 triangle | 4, 5 path on 4: end, interior | 6, 7 claw: leaf, centre |
 *     8 4-cycle | 9, 10, 11 paw: pendant, triangle node off the tail, triangle node carrying the tail |
 *     12, 13 diamond: degree-2 node, degree-3 node (on the chord) | 14 4-clique
 *   No induced subgraph is enumerated: the non-induced counts N0 .. N14 per node come from d(v), t(e) = the triangles
 *   through edge e, t(v) = 1/2 sum_u t(vu), S1(v) = sum_u (d(u) - 1), Q(v) = the 4-cycles through v and K4(v) = the
 *   4-cliques at v (u over the neighbours of v)
 *     N0 = d   N1 = S1   N2 = C(d, 2)   N3 = t(v)   N4 = sum_u (S1(u) - (d(v) - 1)) - 2 t(v)
 *     N5 = sum_u ((d(v) - 1)(d(u) - 1) - t(vu))   N6 = sum_u C(d(u) - 1, 2)   N7 = C(d, 3)   N8 = Q(v)
 *     N9 = sum_u (t(u) - t(uv))   N10 = sum_u t(vu)(d(u) - 2)   N11 = t(v)(d(v) - 2)
 *     N12 = sum over the triangles {v, u, w} of (t(uw) - 1)   N13 = sum_u C(t(vu), 2)   N14 = K4(v)
 *   and the orbits follow by back-substitution through a fixed unit upper-triangular integer matrix (N = A o; the table
 *   is in csrc/grx_graphlets.hip), integer subtraction only.
 *   d_row_ptr / d_col: the CSR of the distinct arcs of an undirected graph, grx_truss_numbers' contract: SYMMETRIC,
 *   columns ascending and distinct inside a row, no diagonal entry; n < 2^31, nnz = row_ptr[n] even and < 2^31.  Rows
 *   longer than GRX_HUB_FACTOR * lanes_per_row (4, 8, 16 or 32) must be listed in d_hub_rows (the row passes' launch
 *   shape; the intersections have no hub path).
 *   d_o_row_ptr / d_o_col: an acyclic orientation of the same graph with ascending out-rows, one arc of every edge
 *   (o_row_ptr[n] = nnz / 2): the degree orientation of grx_orient_count / grx_orient_fill, whose out-rows are bounded
 *   by sqrt(2 m) whatever the hubs' degrees.
 *   d_squares: int64[n], Q: d_squares of grx_square_clustering on the same CSR.
 *   d_orbits: int64[15][n], overwritten, one contiguous column per orbit.  d_noninduced: int64[15][n] or NULL, the N.
 *   d_arc_triangles: int32[nnz] or NULL, t(e) at BOTH arcs of the edge.
 *   Method: see the header of csrc/grx_graphlets.hip.  Cost: two row intersections per edge (t(e); the N12 pass only
 *   for the edges with a triangle), each min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers, four row
 *   passes, and the 4-clique listing on the orientation: per oriented triangle min(d+(u), d+(v), d+(w)) * 2 ceil(log2
 *   max d+) dependent 4-byte gathers, one 64-bit integer atomic per 4-clique found, at most one more per triangle and
 *   two per arc.
 *   Exact: integer atomics only and no result depends on their order, so every output has the same bits in every run,
 *   for every lanes_per_row and for every relabelling of the rows.  The row sums are carried in doubles that hold
 *   integers: the outputs are exact while every N is below 2^53; the final arithmetic is int64.
 *   d_workspace: grx_graphlet_orbits_workspace_bytes(n, nnz) bytes (80 n + 12 nnz: ten int64 per node and three int32
 *   per arc, each array rounded up to 256 bytes).  n == 0: GRX_OK with nothing launched; nnz == 0: the outputs are
 *   zeroed.  Otherwise the call reads row_ptr[n] and o_row_ptr[n] back to check them and so waits for the stream
 *   once, before its first launch.
 */
size_t grx_graphlet_orbits_workspace_bytes(int64_t n, int64_t nnz);
int grx_graphlet_orbits(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int64_t *d_o_row_ptr,
                        const int32_t *d_o_col, const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row,
                        const int64_t *d_squares, int64_t *d_orbits, int64_t *d_noninduced, int32_t *d_arc_triangles,
                        void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_triad_census: the triad census of a directed graph per node (Holland and Leinhardt 1970; networkx's
 *   triadic_census): for each of the 16 isomorphism classes of three nodes with their arcs, the number of triads of
 *   that class that contain the node.  Columns in networkx's order:
 *     0 003 | 1 012 | 2 102 | 3 021D | 4 021U | 5 021C | 6 111D | 7 111U | 8 030T | 9 030C | 10 201 | 11 120D |
 *     12 120U | 13 120C | 14 210 | 15 300
 *   d_row_ptr / d_col: the STRUCTURALLY SYMMETRIC CSR of all neighbours (predecessors and successors): columns
 *   ascending and distinct inside a row, no diagonal entry; n < 2^31.  Rows longer than GRX_HUB_FACTOR * lanes_per_row
 *   (4, 8, 16 or 32) must be listed in d_hub_rows (the row passes' launch shape; the intersections have no hub path).
 *   d_codes: uint8[nnz], the direction code of arc slot (u, v): 1 = only u -> v, 2 = only v -> u, 3 = both; the code at
 *   (v, u) is the mirror of the one at (u, v).  Only the two low bits are read.
 *   d_census: int64[16][n], overwritten, one contiguous column per type.  d_totals: int64[16] or NULL, the census of
 *   the graph: the column sums divided by 3, summed on the device in integers.  d_arc_triads: int32[nnz] or NULL, the
 *   common neighbours of the pair (the closed triads through it) at BOTH slots of the pair.
 *   Method: see the header of csrc/grx_triads.hip: only the closed triads are enumerated, the open ones follow from
 *   the neighbour classes by a fixed 7 x 6 integer matrix and the dyadic ones from degrees and common neighbours.
 *   Cost: one row intersection per adjacent pair (min(d_u, d_v) * ceil(log2 max(d_u, d_v)) dependent 4-byte gathers),
 *   two one-byte gathers and six 64-bit integer atomics per closed triad, two row passes.
 *   Exact: integer atomics only and no result depends on their order, so every output has the same bits in every run,
 *   for every lanes_per_row and for every relabelling of the rows.  The row sums are carried in doubles that hold
 *   integers: the outputs are exact while every intermediate (C(n - 1, 2); a sum of degrees over a row) is below 2^53;
 *   the final arithmetic is int64.
 *   d_workspace: grx_triad_census_workspace_bytes(n, nnz) bytes (40 n + 8 nnz: five 8-byte vectors per node and two
 *   int32 per arc, each array rounded up to 256 bytes).  n == 0: GRX_OK with nothing launched; nnz == 0: column 003 is
 *   C(n - 1, 2).  Otherwise the call reads row_ptr[n] back and so waits for the stream once, before its first launch.
 */
size_t grx_triad_census_workspace_bytes(int64_t n, int64_t nnz);
int grx_triad_census(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const uint8_t *d_codes,
                     const int32_t *d_hub_rows, int64_t n_hub_rows, int lanes_per_row, int64_t *d_census,
                     int64_t *d_totals, int32_t *d_arc_triads, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_neighbor_roles: the neighbour-role table of RolX NeighborSense (Henderson et al., KDD 2012, section 4), the
 *   sparse x dense product N = A P of a CSR with the node x role memberships P.  For row i with the arcs at positions
 *   p = row_ptr[i] .. row_ptr[i + 1] - 1
 *     GRX_NEIGHBOR_SUM :  N[k, i] = sum_p w_p * P[col_p, k]
 *     GRX_NEIGHBOR_MEAN:  that sum divided by D(i) = sum_p w_p; 0.0 where D(i) == 0 (a row without arcs, a row of zero
 *                         strength): never NaN for finite input
 *   d_w: fp64[nnz] or NULL (every w_p = 1: no product is formed and D(i) = the number of arcs, exact).
 *   d_P: fp64, n x r row-major with leading dimension ldp >= r (P[v, k] = d_P[v * ldp + k]); 1 <= r <= GRX_MAX_ROLES.
 *   d_out: fp64, FEATURE-major r x n with leading dimension ld_out >= n (N[k, i] = d_out[k * ld_out + i]), the layout
 *   grx_gram reads; every entry of the r rows is overwritten, nothing beyond column n is touched.
 *   Summation order, the same for every role k and for D(i): let d be the number of arcs of the row and S = 8 slots if
 *   d <= 1024, S = 128 slots otherwise.  Slot s starts from +0.0 and adds the terms of the arcs row_ptr[i] + s,
 *   row_ptr[i] + s + S, row_ptr[i] + s + 2 S, ... in that order, each product w_p * P[col_p, k] rounded on its own
 *   before it is added (no fused multiply-add).  Then for h = S / 2, S / 4, ..., 1: slot[t] = slot[t] + slot[t + h]
 *   for every t < h; slot[0] is the sum.  The mean is one division of that sum by D(i), itself the w_p summed in the
 *   same slots and the same tree.  The order depends on the positions of the row's arcs only -- not on the run, the
 *   grid or lanes_per_row -- so every output has the same bits in every call; there are no floating-point atomics.
 *   lanes_per_row: the lanes that walk one row, S * CL.  CL = ceil(r / 2) rounded up to a power of two (1 .. 16) lanes
 *   fetch one membership row together, two columns each; S = 1, 2, 4 or 8 physical arc slots carry the 8 slots of the
 *   order above, 8 / S of them per lane.  0 = the library's choice (S = min(8, 32 / CL)), otherwise CL times 1, 2, 4
 *   or 8 and at most 64; every accepted value gives the same bits.
 *   Method: see the header of csrc/grx_neighbor_sense.hip.  Two launches, no workspace, no device -> host read;
 *   rows longer than 1024 arcs are walked by a whole workgroup each, in the second launch.  Cost: per arc one gathered membership row of 8 r bytes.
 *   n == 0 returns GRX_OK at once.  GRX_ERR_INVALID before any HIP call for n outside [0, 2^31), r < 1, ldp < r,
 *   ld_out < n, another mode or lanes_per_row, or a NULL pointer (d_w excepted); GRX_ERR_UNSUPPORTED for
 *   r > GRX_MAX_ROLES.  Column indices are trusted to lie in [0, n).
 */
#define GRX_NEIGHBOR_SUM 0
#define GRX_NEIGHBOR_MEAN 1
int grx_neighbor_roles(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const double *d_w,
                       const double *d_P, int64_t ldp, int r, int mode, int lanes_per_row, double *d_out,
                       int64_t ld_out, void *stream);

/*
 * grx_similar_rows: structural similarity (Henderson et al., KDD 2012, section 5.2) -- for every query row its k
 *   nearest candidate rows of a node x column table, exactly.  Memberships, ReFeX features or the output of a
 *   transform: any fp64 table of 1 <= c <= GRX_MAX_ROLES columns.
 *   d_X: the n candidates, row-major with leading dimension ldx >= c; d_Q: the nq queries, ldq >= c; d_Q may alias d_X.
 *   d_self: int32[nq] or NULL -- the candidate row left out for query q (its own row when a table queries itself),
 *   -1 = none.  It is left out by position: a duplicate of the query is a legitimate neighbour.
 *     GRX_SIMILARITY_COSINE   : larger is nearer.  norm(x) = sqrt(sum_j x_j * x_j), xn_j = x_j / norm (0.0 for a row of
 *                               norm 0: its score with anything is 0.0), score = sum_j qn_j * xn_j.
 *     GRX_SIMILARITY_EUCLIDEAN: smaller is nearer.  Ordered by d2 = sum_j (q_j - x_j) * (q_j - x_j); the score reported
 *                               is sqrt(d2).
 *   Arithmetic: every sum runs j = 0 .. c - 1 from +0.0, every product and difference is rounded on its own before it
 *   is added (no fused multiply-add), the normalisation is one division per element by the rounded norm.  So the score
 *   of a pair has the same bits for every `segments`, in every run, and score(a, b) == score(b, a) bitwise.
 *   d_index int32, d_score fp64: [nq, k] row-major with leading dimension ld_out >= k.  Row q holds the first k
 *   candidates in the strict total order (score nearer first, then smaller candidate row), d_self[q] left out; the
 *   result is unique.  With fewer than k candidates the remaining slots hold index -1 and score NaN.  Nothing beyond
 *   column k of a row is touched.  No floating-point atomics.
 *   segments: 0 = the library's choice; otherwise the candidates are split into that many contiguous ranges (at most one
 *   per 64-row candidate tile, at most 1024), each scanned by its own workgroups, and the per-range lists are merged by
 *   one more launch.  This is what fills the chip when nq is small.  The result does not depend on it.
 *   d_workspace: grx_similar_rows_workspace_bytes(n, nq, c, k, segments) bytes: the normalised, zero-padded copies of X
 *   and Q and the lists of the segments.
 *   Non-finite input is the caller's to refuse; a NaN key is never taken, nothing hangs or leaves its buffers.
 *   Limits: n, nq < 2^31, 1 <= k <= GRX_MAX_TOPK.  nq == 0 returns GRX_OK at once; n == 0 fills the slots that exist
 *   (index -1, score NaN: one small launch, none when the outputs are NULL) and returns GRX_OK.  GRX_ERR_UNSUPPORTED for
 *   c > GRX_MAX_ROLES; GRX_ERR_INVALID before any HIP call for n, nq, k or c < 1 out of range, ldx < c, ldq < c,
 *   ld_out < k, another metric, segments < 0, a workspace that is too small, or a NULL pointer (d_self excepted) with
 *   n and nq positive.  Method, LDS budget and bound: the header of csrc/grx_similarity.hip.
 */
#define GRX_MAX_TOPK 64
#define GRX_SIMILARITY_COSINE 0
#define GRX_SIMILARITY_EUCLIDEAN 1
size_t grx_similar_rows_workspace_bytes(int64_t n, int64_t nq, int c, int k, int segments);
int grx_similar_rows(int64_t n, int c, const double *d_X, int64_t ldx, int64_t nq, const double *d_Q, int64_t ldq,
                     const int32_t *d_self, int k, int metric, int segments, int32_t *d_index, double *d_score,
                     int64_t ld_out, void *d_workspace, size_t workspace_bytes, void *stream);

/*
 * grx_components: the connected components of an undirected graph, or the weakly or the strongly connected components
 *   of a directed one -- networkx.connected_components, weakly_connected_components, strongly_connected_components
 *   (networkx/algorithms/components) -- as one label per node.
 *   d_row_ptr / d_col: the CSR of the graph's distinct arcs, rows in any order; self-loop entries are allowed and change
 *   nothing; weights are not read.  Rows longer than GRX_HUB_FACTOR * lanes_per_row (in_lanes_per_row) must be listed
 *   in d_hub_rows (d_in_hub_rows).
 *   mode: GRX_COMPONENTS_CONNECTED -- the CSR is symmetric (every edge from both ends), all d_in_* NULL / 0;
 *         GRX_COMPONENTS_WEAK      -- the out-CSR of a directed graph alone; d_in_* are ignored and may be NULL;
 *         GRX_COMPONENTS_STRONG    -- the out-CSR and d_in_row_ptr / d_in_col, its transpose (GRX_ERR_INVALID without).
 *   Method: CONNECTED and WEAK by the lock-free union-find of grx_biconnected (hook the larger root under the smaller,
 *   pointer jumping, flatten); STRONG by trim and colour (Orzan 2004; Barnat et al. 2011): trim the nodes without an
 *   alive in- or out-neighbour, propagate the smallest id forward to a fixed point, close backward from the nodes that
 *   kept their own id inside their colour, remove what was reached, repeat -- device-steered rounds, 16 per read-back;
 *   see the header of csrc/grx_components.hip for the rounds, the bound and the known worst case (a chain of small
 *   components with ascending ids: one outer iteration per component).
 *   d_label: int32[n], overwritten: the smallest row id of v's component.
 *   d_size:  int64[n] or NULL: the number of rows in v's component.
 *   n_components: HOST int64 or NULL (reading it waits for the stream).
 *   h_rounds: HOST int64 or NULL: the number of rounds STRONG ran (0 for the other modes).
 *   Exact (integers only; vector integer atomics whose results do not depend on their order): every output has the
 *   same bits in every run and for every lane width, and is the same partition under every relabelling of the rows.
 *   0 <= n < 2^31; n == 0 returns GRX_OK at once with 0 components.  d_workspace: grx_components_workspace_bytes(n)
 *   bytes (about 16 n).  STRONG waits for the stream.
 *
 * grx_reachable: the closure of a seed set along the CSR's arcs.  d_flag: int32[n], in and out: non-zero on entry marks
 *   a seed; on return 1 for every seed and every node reachable from one, 0 elsewhere (descendants with the out-CSR,
 *   ancestors with the in-CSR).  Level-synchronous, 16 levels per read-back.  h_count: HOST int64 or NULL, the number
 *   of ones; h_levels: HOST int64 or NULL, the depth reached (0 when the seeds reach nothing new).  Conventions, limits
 *   and exactness as above.  d_workspace: grx_reachable_workspace_bytes(n) bytes (about 4 n).  The call waits for the
 *   stream.
 */
enum { GRX_COMPONENTS_CONNECTED = 0, GRX_COMPONENTS_WEAK = 1, GRX_COMPONENTS_STRONG = 2 };
size_t grx_components_workspace_bytes(int64_t n);
int grx_components(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                   int64_t n_hub_rows, int lanes_per_row, const int64_t *d_in_row_ptr, const int32_t *d_in_col,
                   const int32_t *d_in_hub_rows, int64_t n_in_hub_rows, int in_lanes_per_row, int mode,
                   int32_t *d_label, int64_t *d_size, int64_t *n_components, int64_t *h_rounds,
                   void *d_workspace, size_t workspace_bytes, void *stream);

size_t grx_reachable_workspace_bytes(int64_t n);
int grx_reachable(int64_t n, const int64_t *d_row_ptr, const int32_t *d_col, const int32_t *d_hub_rows,
                  int64_t n_hub_rows, int lanes_per_row, int32_t *d_flag, int64_t *h_count, int64_t *h_levels,
                  void *d_workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GRX_H */
