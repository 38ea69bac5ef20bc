/*
 * fa_hip.h — C ABI of the MI355X (gfx950) flash-attention library.
 *
 * Drop-in boundary for the hot path of nikopj/FlashAttention.jl
 * (reference mounted read-only at /root/reference; citations are path:line
 * inside it).  The Julia host code binds these symbols with `ccall`
 * (INTEGRATION.md); the Python ctypes mirror in flashattention.jl_amd/fa_hip
 * binds the very same symbols, so parity evidence transfers.
 *
 * Layout contract (all entry points): the reference's Julia column-major
 * layout with contiguous batch.  A 3-D array X of Julia shape (N, d, B) sits
 * at element offset  n + N*k + N*d*b  (src/dense.jl:6-8 flattens spatial dims
 * into N).  l and m are (N, 1, B): offset n + N*b.  There is no separate head
 * dimension: (batch, heads) of the benchmark configs are one batch of B*H
 * (SURVEY.md §8a).
 *
 * Every pointer is a DEVICE pointer owned by the caller.  Inputs are read
 * only; outputs are fully written (the callee initialises, as
 * src/dense.jl:58-60 does).  `hip_stream` is a hipStream_t (NULL = default
 * stream).  Calls are asynchronous on that stream, stateless, and safe from
 * concurrent host threads on distinct streams.  No call allocates device
 * memory, synchronises, or aborts: each returns FA_OK (0) or a nonzero
 * fa_status, with a thread-local message in fa_last_error().  A workspace
 * belongs to one call at a time: calls that may run concurrently (distinct
 * streams) need distinct workspaces (the backward kernels keep hand-off
 * counters and strip counters in theirs).  A workspace may start at any
 * address: the *_workspace() sizes include 256 bytes of slack, and every entry
 * point rounds the addresses of its counters and staging buffers up to 256 B
 * inside it.
 */
#ifndef FA_HIP_H
#define FA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FA_HIP_ABI_VERSION 1

/* Element type of Q, K, V, O (and dO, dQ, dK, dV).  l, m are always float32
 * (documented deviation: the reference keeps them in T, src/dense.jl:12-13).
 * FA_DTYPE_F64 is the element type of the reference's own tests and timings
 * (test/test.jl:12, logs/compare1.txt): dense forward / backward, the windowed
 * forward / backward, window / unwindow, circulant and softmax accept it; it runs
 * fp64 SIMT parity kernels, and its backward recomputes the row statistics in
 * double instead of reading the float32 l, m. */
typedef enum fa_dtype {
    FA_DTYPE_F32  = 0,
    FA_DTYPE_BF16 = 1,
    FA_DTYPE_F16  = 2,
    FA_DTYPE_F64  = 3
} fa_dtype;

typedef enum fa_status {
    FA_OK                = 0,
    FA_ERR_INVALID_ARG   = 1, /* bad pointer / size / dtype (reference: DimensionMismatch) */
    FA_ERR_UNSUPPORTED   = 2, /* valid but unsupported (e.g. head dim > fa_max_head_dim()) */
    FA_ERR_HIP           = 3, /* HIP launch / runtime error */
    FA_ERR_WORKSPACE     = 4  /* workspace missing or too small */
} fa_status;

/* Dense forward.  Replaces the body of
 *   dense_fa!(O, l, m, Q, K, V)          src/dense.jl:21-102
 * (and, with caller-side allocation, dense_fa(q, k, v), src/dense.jl:1-19).
 *   Q (N, d, B), K (Nk, d, B), V (Nk, dv, B)  ->  O (N, dv, B),
 *   l (N, 1, B) = sum_j exp(s_ij - m_i),  m (N, 1, B) = max_j s_ij,
 *   s = scale * Q K^T  (natural-log units, as src/dense.jl:78-91).
 * scale <= 0 selects the reference's tau = 1/sqrt(d) (src/dense.jl:43).
 * The reference requires Nk == N and dv == d (Appendix A.1); both are lifted.
 * Empty inputs behave as dense_fa! does with empty arrays: N == 0 or B == 0 is a
 * no-op (no pointer is dereferenced); Nk == 0 writes O = 0, l = 0, m = -Inf, the
 * initial state of src/dense.jl:58-60.  d, dv must be >= 1. */
int fa_dense_fwd(int dtype,
                 const void* Q, const void* K, const void* V,
                 void* O, float* l, float* m,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                 float scale, void* hip_stream);

/* fa_dense_fwd with a caller-owned workspace (same contract otherwise).  For
 * bf16 / fp16 with Nk % 8 != 0 the workspace holds zero-padded K / V copies of
 * row stride roundup(Nk, 8), so the ragged shape runs the fast MFMA kernels
 * instead of the generic one (3.6-6x).  workspace may be NULL
 * when fa_dense_fwd_workspace() returns 0. */
int fa_dense_fwd_ws(int dtype,
                    const void* Q, const void* K, const void* V,
                    void* O, float* l, float* m,
                    int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                    float scale, void* workspace, size_t workspace_bytes,
                    void* hip_stream);

/* Workspace bytes fa_dense_fwd_ws needs for these sizes (0 is a valid answer). */
size_t fa_dense_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                              int64_t dv, int64_t batch);

/* Workspace bytes fa_dense_bwd needs for these sizes (0 is a valid answer):
 * a 256-B header (fa_dense_bwd_handoff_status), 8·N·batch bytes of row
 * statistics; for bf16 / fp16 shapes outside the MFMA kernels' set, zero-padded
 * copies; and when the single-pass kernel applies (grids that
 * fill the chip), per-slice counters plus the running fp32 dQ sums of the two
 * chains per slice, 2·4·N·d·batch bytes (17.2 GB for configs[4]'s 1024 slabs of
 * (16384, 128)).  A
 * smaller workspace that still holds the first parts (the size this function
 * returns under fa_debug_set_bwd_mode(1)) runs the two-pass form instead.  The
 * answer depends on the current device's CU count. */
size_t fa_dense_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                              int64_t dv, int64_t batch);

/* Dense backward.  Replaces dense_fa_backward(Q, K, V, O, dO, l, m)
 * (src/dense.jl:104-167; executable spec OneDFastBack,
 * src_cpp/FlashAttention.cpp:194-252):
 *   P = exp(s - m)/l, dV = P^T dO, dP = dO V^T, D = rowsum(dO .* O),
 *   dS = P .* (dP - D), dQ = scale dS K, dK = scale dS^T Q.
 * l, m are the forward's outputs.  dQ, dK, dV are fully written, without
 * atomics.  dK and dV are bitwise reproducible.  dQ is bitwise reproducible
 * whenever the single pass's ordered dQ hand-off completes (it sums each query
 * slice over the key blocks in a fixed order).  Every hand-off wait is on a
 * workgroup dispatched earlier in the same launch, so no co-residency is needed:
 * other streams or processes sharing the GPU slow the call down but do not make it
 * give up.  A wait gives up only as a safety net, when neither the launch's arrival
 * count nor any member of the waiting slab has made progress for
 * FA_BWD_HANDOFF_STALL_US microseconds (100 ms); dQ of that slab is then recomputed
 * by a separate pass that sums in a different order: same values within rounding,
 * not the same bits, and slower.  fa_dense_bwd_handoff_status reports whether any
 * slab did. */
#define FA_BWD_HANDOFF_STALL_US 100000
int fa_dense_bwd(int dtype,
                 const void* Q, const void* K, const void* V,
                 const void* O, const void* dO,
                 const float* l, const float* m,
                 void* dQ, void* dK, void* dV,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                 float scale, void* workspace, size_t workspace_bytes,
                 void* hip_stream);

/* Diagnostic for the call that last used `workspace` in fa_dense_bwd: reads the
 * workspace header (synchronises hip_stream, so call it after that backward on the
 * same stream).  *status = -1: that call ran the two-pass form (no hand-off),
 * 0: single pass, every dQ hand-off completed, 1: single pass, some slab's hand-off
 * gave up and its dQ was recomputed (see fa_dense_bwd).  FA_ERR_INVALID_ARG if the workspace
 * holds no fa_dense_bwd header. */
int fa_dense_bwd_handoff_status(const void* workspace, size_t workspace_bytes,
                                void* hip_stream, int* status);

/* Windowed forward.  Replaces windowed_fa(q, k, v, ws; stride, pad)
 * (src/windowed.jl:3-23; block_fa = stride ws, src/windowed.jl:1), fusing
 * window (src/utils.jl:36-44) -> dense_fa -> unwindow / divisor
 * (src/utils.jl:46-54, src/windowed.jl:16-19) into one pass.
 *   q, k: (S_1, ..., S_k, d, B);  v: (S_1, ..., S_k, dv, B)
 *   y:    (S_1, ..., S_k, dv, B)  (pixels no window covers are NaN, as in
 *                                  the reference, Appendix A.7)
 *   l, m: (ws^k, 1, L, B) window layout (src/windowed.jl:20-21),
 *         L = prod_i ((S_i + 2 pad - ws) / stride + 1).
 * nspatial = k in 1..3; pad < 0 selects the reference default (ws-1)/2.
 * B == 0 (an empty batch) is a no-op after the geometry is validated; the
 * same holds for fa_window, fa_unwindow and fa_windowed_bwd. */
int fa_windowed_fwd(int dtype,
                    const void* q, const void* k, const void* v,
                    void* y, float* l, float* m,
                    int nspatial, const int64_t* spatial,
                    int64_t d, int64_t dv, int64_t batch,
                    int64_t ws, int64_t stride, int64_t pad,
                    float scale, void* workspace, size_t workspace_bytes,
                    void* hip_stream);

/* Workspace bytes fa_windowed_fwd needs (0 is a valid answer: the fused
 * single-pass kernel needs none; large windows / fp32 use a composed
 * gather -> dense -> fold path that stages windows in the workspace). */
size_t fa_windowed_fwd_workspace(int dtype, int nspatial, const int64_t* spatial,
                                 int64_t d, int64_t dv, int64_t batch,
                                 int64_t ws, int64_t stride, int64_t pad);

/* window(x, ws; stride, pad) — reference src/utils.jl:36-45 (NNlib.unfold):
 * x (S_1..S_k, C, batch) -> xw (ws^k, C, L, batch), zero padding outside the
 * image, window token order first-spatial-dim fastest.  xw fully written. */
int fa_window(int dtype, const void* x, void* xw,
              int nspatial, const int64_t* spatial, int64_t C, int64_t batch,
              int64_t ws, int64_t stride, int64_t pad, void* hip_stream);

/* unwindow(xw, size(x), ws; stride, pad) — reference src/utils.jl:47-54
 * (NNlib.fold): xw (ws^k, C, L, batch) -> x (S_1..S_k, C, batch), the SUM over
 * overlapping windows (0 where no window covers a pixel).  Deterministic (one
 * thread per output pixel, fixed window order).  x fully written. */
int fa_unwindow(int dtype, const void* xw, void* x,
                int nspatial, const int64_t* spatial, int64_t C, int64_t batch,
                int64_t ws, int64_t stride, int64_t pad, void* hip_stream);

/* Workspace bytes fa_windowed_bwd needs. */
size_t fa_windowed_workspace(int dtype, int nspatial, const int64_t* spatial,
                             int64_t d, int64_t dv, int64_t batch,
                             int64_t ws, int64_t stride, int64_t pad);

/* Windowed backward (README.md:36-37 claims it, no code
 * exists in the reference): the exact chain rule of windowed_fa.
 * y, l, m are fa_windowed_fwd's outputs; dq, dk, dv fully written. */
int fa_windowed_bwd(int dtype,
                    const void* q, const void* k, const void* v,
                    const void* y, const void* dy,
                    const float* l, const float* m,
                    void* dq, void* dk, void* dv_,
                    int nspatial, const int64_t* spatial,
                    int64_t d, int64_t dv, int64_t batch,
                    int64_t ws, int64_t stride, int64_t pad,
                    float scale, void* workspace, size_t workspace_bytes,
                    void* hip_stream);

/* Circulant (periodic banded) attention, replaces
 *   circulant_fa!(O, l, m, Q, K, V, W)   reference src/circulant.jl:9-118
 * (naive form circulant_dpa! src/naive/circulant.jl:8-36).  Query i attends
 * the W band entries (i - p + t) mod N, t = 0..W-1, p = (W-1)/2 — the keys
 * cartesian_circulant enumerates (src/utils.jl:6-17); W > N repeats keys.
 * Q, K: (N, d, batch); V: (N, dv, batch); O: (N, dv, batch); l, m: (N, 1, batch)
 * float32 with the dense_fa! meaning.  Any W >= 1 (the reference's own
 * benchmark uses even W, bench/compare.jl:98).  N == 0 or batch == 0 is a
 * no-op (the reference's row and batch loops run zero times). */
int fa_circulant_fwd(int dtype, const void* Q, const void* K, const void* V,
                     void* O, float* l, float* m,
                     int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W,
                     float scale, void* hip_stream);

/* Workspace bytes fa_circulant_bwd needs: the per-query row statistics (two
 * float arrays of N·batch, double for FA_DTYPE_F64), each rounded up to 256 B,
 * plus 256 B of slack so the workspace may start at any address. */
size_t fa_circulant_bwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv,
                                  int64_t batch, int64_t W);

/* Circulant backward (the reference has none): the chain rule of
 * fa_circulant_fwd over the same band, j(i, t) = (i - p + t) mod N:
 *   P_it = exp(scale q_i.k_j - m_i)/l_i, dP_it = dO_i.v_j, D_i = dO_i.O_i,
 *   dS_it = P_it (dP_it - D_i), dQ_i = scale sum_t dS_it k_j,
 *   dK_j = scale sum_{(i,t)->j} dS_it q_i, dV_j = sum_{(i,t)->j} P_it dO_i.
 * W > N repeats keys; every band entry counts once.  O, l, m are the forward's
 * outputs (FA_DTYPE_F64 recomputes the row statistics in double and does not
 * read l, m).  dQ, dK, dV are fully written, without atomics, and all three
 * are bitwise reproducible: no sum crosses a workgroup.  N == 0 or batch == 0
 * is a no-op.  Head dims above fa_max_head_dim() and extents past the kernels'
 * 32-bit addressing give FA_ERR_UNSUPPORTED, a missing or short workspace
 * FA_ERR_WORKSPACE, both before any launch. */
int fa_circulant_bwd(int dtype,
                     const void* Q, const void* K, const void* V,
                     const void* O, const void* dO,
                     const float* l, const float* m,
                     void* dQ, void* dK, void* dV,
                     int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t W,
                     float scale, void* workspace, size_t workspace_bytes,
                     void* hip_stream);

/* Causal dense attention (the reference has none; NNlib.dot_product_attention's
 * causal mask, bottom-right aligned): query i attends the keys j <= i + off,
 * off = Nk - N, so the last query sees every key (a KV cache's alignment) and
 * N == Nk is the ordinary lower triangle.
 *   Q (N, d, B), K (Nk, d, B), V (Nk, dv, B) -> O (N, dv, B); l, m (N, 1, B)
 * float32 with the dense_fa! meaning, taken over the visible keys only.  The mask
 * is a select (score := -Inf), not an added bias: a masked key's K values reach no
 * result (inputs are assumed finite: a masked V is multiplied by P = 0).  dv != d,
 * any d, dv <= fa_max_head_dim(), ragged N / Nk and all four dtypes are accepted, as
 * for fa_dense_fwd_ws.  Checks, in order: null pointers, DimensionMismatch, head
 * dims and Nk >= N (Nk < N, where some query would see no key, is
 * FA_ERR_UNSUPPORTED), 32-bit extents, workspace; all before any launch.  N == 0
 * or batch == 0 is a no-op.  The same tile bodies as the dense forward with the key
 * loop cut at each workgroup's diagonal; causal launches never split the keys and
 * never take the one-wave-per-SIMD kernel. */
int fa_causal_fwd(int dtype,
                  const void* Q, const void* K, const void* V,
                  void* O, float* l, float* m,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                  float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream);

/* Workspace bytes fa_causal_fwd needs (0 is a valid answer): the zero-padded K / V
 * copies for bf16 / fp16 with Nk % 8 != 0, as fa_dense_fwd_ws, plus 256 B of slack
 * so the workspace may start at any address.  No split-KV part. */
size_t fa_causal_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                               int64_t dv, int64_t batch);

/* Workspace bytes fa_causal_bwd needs: the 256-B header, the row statistics
 * (8·N·batch bytes, double for FA_DTYPE_F64) and, for bf16 / fp16 shapes outside
 * the MFMA kernels' set, the zero-padded copies, plus 256 B of slack so the
 * workspace may start at any address.  Never the single pass's running sums, and
 * independent of the device. */
size_t fa_causal_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                               int64_t dv, int64_t batch);

/* Causal backward: the chain rule of fa_causal_fwd over the visible keys,
 *   P_ij = exp(s_ij - m_i)/l_i for j <= i + off (0 elsewhere), dV = P^T dO,
 *   dP = dO V^T, D = rowsum(dO .* O), dS = P .* (dP - D), dQ = scale dS K,
 *   dK = scale dS^T Q.
 * O, l, m are fa_causal_fwd's outputs (FA_DTYPE_F64 recomputes the statistics in
 * double and does not read l, m).  It always runs the two-pass form (a dQ pass whose
 * key tiles end at the diagonal, a dK/dV pass whose query tiles begin there) and
 * never fa_dense_bwd's single pass: the ordered dQ hand-off's rotated chains assume
 * every member visits every slice, and under a causal mask the hand-off costs more
 * than it saves.  The two passes need no atomics and no hand-off, so dQ, dK and dV
 * are ALL bitwise reproducible.  The workspace header is written so that
 * fa_dense_bwd_handoff_status on this workspace answers -1.  dQ, dK, dV are fully
 * written.  Checks and empty inputs as fa_causal_fwd. */
int fa_causal_bwd(int dtype,
                  const void* Q, const void* K, const void* V,
                  const void* O, const void* dO,
                  const float* l, const float* m,
                  void* dQ, void* dK, void* dV,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                  float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream);

/* Local (sliding-window) attention: a window (left, right) around the causal
 * diagonal.  With off = Nk - N (bottom-right alignment, as fa_causal_fwd), query i
 * attends the keys j with
 *   0 <= j < Nk   and   i + off - left <= j <= i + off + right.
 * left < 0 means no left bound, right < 0 no right bound, and a value >= Nk is the
 * same as unbounded (both are int64_t and are clamped before any 32-bit use):
 * (-1, 0) is fa_causal_fwd's mask, (-1, -1) fa_dense_fwd's, and (0, 0) lets query i
 * see key i + off only.  Nk < N is FA_ERR_UNSUPPORTED; with Nk >= N the key i + off
 * exists, so every query sees at least one key.  The mask is a select (score :=
 * -Inf), never an added bias; l and m (float32 for every dtype) are taken over the
 * visible keys.  Shapes, dtypes, head dims, ragged N / Nk, the order of the checks
 * (null pointers, DimensionMismatch, head dims and Nk >= N, 32-bit extents,
 * workspace; all before any launch) and the empty cases (N == 0 or batch == 0 is a
 * no-op) are fa_causal_fwd's.  A local call always runs the local instantiations of
 * the kernels, also for (-1, 0) and (-1, -1): the same tile bodies with the key loop
 * cut on both sides per workgroup and per wave; never split-KV, never the
 * one-wave-per-SIMD kernel. */
int fa_local_fwd(int dtype,
                 const void* Q, const void* K, const void* V,
                 void* O, float* l, float* m,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                 int64_t left, int64_t right,
                 float scale, void* workspace, size_t workspace_bytes,
                 void* hip_stream);

/* Workspace bytes fa_local_fwd needs (0 is a valid answer): fa_causal_fwd_workspace's
 * answer for the shape (the padded K / V copies only).  It depends on the shape
 * alone, not on the window or the device. */
size_t fa_local_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                              int64_t dv, int64_t batch);

/* Workspace bytes fa_local_bwd needs: fa_causal_bwd_workspace's answer for the shape
 * (header, row statistics, pad plan).  Independent of the window and the device. */
size_t fa_local_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                              int64_t dv, int64_t batch);

/* Local backward: the chain rule of fa_local_fwd over the visible keys (the
 * formulas of fa_causal_bwd with P_ij = 0 outside the window).  O, l, m are
 * fa_local_fwd's outputs for the same (left, right) (FA_DTYPE_F64 recomputes the
 * statistics in double).  Always the two-pass form: a dQ pass over the key tiles
 * between each block's first query's left edge and its last query's right edge, and
 * a dK/dV pass over the queries j - off - right <= i <= j - off + left that see key
 * j.  A key that no query sees (j < off - left: a KV cache longer than the window)
 * gets dK = dV = 0, actually written: dQ, dK, dV are fully written, and all three are
 * bitwise reproducible (no atomics, no hand-off).  The workspace header is written
 * with plan 0, so fa_dense_bwd_handoff_status on this workspace answers -1.  Checks
 * and empty inputs as fa_local_fwd. */
int fa_local_bwd(int dtype,
                 const void* Q, const void* K, const void* V,
                 const void* O, const void* dO,
                 const float* l, const float* m,
                 void* dQ, void* dK, void* dV,
                 int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                 int64_t left, int64_t right,
                 float scale, void* workspace, size_t workspace_bytes,
                 void* hip_stream);

/* Varlen attention: fa_local_fwd with per-slab lengths in a padded batch (documents of
 * unequal length; decode requests with unequal KV caches).  q_lens and k_lens are DEVICE
 * pointers to `batch` int32 values (`int` is int32_t on every ABI this library builds for; the
 * library asserts it); NULL means "every slab is full on that side".  For slab b:
 *   nq = clamp(q_lens[b], 0, N),  nk = clamp(k_lens[b], 0, Nk),  off_b = nk - nq  (either sign);
 * the slab is the leading nq rows of Q (and O, l, m) and the leading nk rows of K, V: the layout
 * and strides are the (N, Nk) slab's.  Query i < nq attends the keys j with
 *   0 <= j < nk   and   i + off_b - left <= j <= i + off_b + right,
 * a negative or >= Nk side unbounded as for fa_local_fwd: (-1, -1) with lengths is a
 * key-padding mask, (-1, 0) causal per sequence, bottom-right aligned (the KV-cache form).
 * Fully written, exact zeros: rows i >= nq get O = 0, l = 0, m = -Inf (the Nk == 0 state of
 * fa_dense_fwd); so does a query i < nq that sees no key (nk < nq under a right bound, or
 * nk == 0).  The mask is a select: padding rows of Q, K, V may hold anything finite (the
 * assumption fa_causal_fwd makes for a masked V) and change no bit of any output.
 * The lengths are device data and no call synchronises, so they are not validated on the
 * host: the kernels clamp them as above, which keeps every access inside the slab.
 * Shape-level checks, their order and the empty cases are fa_local_fwd's (Nk < N is
 * FA_ERR_UNSUPPORTED, N == 0 or batch == 0 a no-op that dereferences nothing), all before any
 * launch.  A varlen call always runs the varlen instantiations of the kernels (the local
 * bodies with per-slab extents), also with NULL lengths: the key loop is cut per workgroup
 * and per wave by the lengths as well as by the window, so padding is skipped, not merely
 * masked; never split-KV, never the one-wave-per-SIMD kernel. */
int fa_varlen_fwd(int dtype,
                  const void* Q, const void* K, const void* V,
                  void* O, float* l, float* m,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                  const int* q_lens, const int* k_lens,
                  int64_t left, int64_t right,
                  float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream);

/* Workspace bytes fa_varlen_fwd needs (0 is a valid answer): fa_local_fwd_workspace's answer
 * for the shape.  It depends on the shape alone, not on the lengths, the window or the device. */
size_t fa_varlen_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                               int64_t dv, int64_t batch);

/* Workspace bytes fa_varlen_bwd needs: fa_local_bwd_workspace's answer for the shape. */
size_t fa_varlen_bwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d,
                               int64_t dv, int64_t batch);

/* Varlen backward: the chain rule of fa_varlen_fwd over the visible keys, for the same lengths
 * and window.  O, l, m are fa_varlen_fwd's outputs (FA_DTYPE_F64 recomputes the statistics in
 * double).  Always the two-pass form, header plan 0 (fa_dense_bwd_handoff_status answers -1);
 * dQ, dK, dV are fully written and all three are bitwise reproducible.  Exact zeros: dQ rows
 * i >= nq and the rows of queries that see no key; dK, dV rows j >= nk and the rows of keys
 * that no query sees.  An empty row is chosen from the lengths and the window, never from the
 * caller's l, and contributes nothing to any gradient.  Padding rows of Q, K, V and dO may hold
 * anything finite.  Checks and empty inputs as fa_varlen_fwd. */
int fa_varlen_bwd(int dtype,
                  const void* Q, const void* K, const void* V,
                  const void* O, const void* dO,
                  const float* l, const float* m,
                  void* dQ, void* dK, void* dV,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                  const int* q_lens, const int* k_lens,
                  int64_t left, int64_t right,
                  float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream);

/* Decode attention: fa_varlen_fwd's forward with a `group` factor, split over the keys (a few
 * queries per KV slab against a long cache; several query heads sharing one K / V slab).
 * Forward only.  `batch` counts KV slabs: K is (Nk, d, batch), V (Nk, dv, batch); Q is
 * (N, d, batch * group), O (N, dv, batch * group), l and m (N, 1, batch * group) float32.
 * Query slab bq uses KV slab bq / group (the heads of a group are adjacent: with heads fastest
 * in the flattened batch, query head h reads KV head h / group).  q_lens and k_lens are DEVICE
 * pointers to `batch` int32 values, one per KV slab, shared by its `group` query slabs; NULL
 * means full; they are clamped on the device exactly as for fa_varlen_fwd and never read or
 * validated on the host.  Mask, l, m, O and the empty-row rule are fa_varlen_fwd's: per KV
 * slab nq, nk, off = nk - nq and the window as there; query i < nq sees key j iff 0 <= j < nk
 * and i + off - left <= j <= i + off + right; rows i >= nq and queries that see no key get
 * O = +0, l = 0, m = -Inf, by select; padding rows of Q, K, V may hold anything finite and
 * change no output bit.
 * Limits: N * group <= 32 (all rows of a KV slab are one 32-row MFMA tile; more is
 * FA_ERR_UNSUPPORTED: use fa_varlen_fwd); FA_DTYPE_BF16 and FA_DTYPE_F16 only (F32, F64:
 * FA_ERR_UNSUPPORTED); 1 <= d, dv <= fa_max_head_dim().
 * Checks, in order, all before any launch: null pointers; DimensionMismatch (group < 1
 * included); head dims, Nk >= N, N * group <= 32 and dtype (FA_ERR_UNSUPPORTED); the
 * kernels' 32-bit extents (a K / V slab below 2^31 bytes); the workspace.  N == 0 or
 * batch == 0 is a no-op that dereferences nothing.
 * K and V are never copied: Nk % 8 != 0, or a K / V pointer that is not 16-B aligned, selects
 * an instantiation with narrower loads (slower, correct, no workspace slabs).  Each KV slab's
 * visible key range is cut into the plan's number of equal shares, one workgroup each; the
 * partial results are merged in a fixed order (no atomics, no hand-off between workgroups), so
 * all outputs are bitwise reproducible for given lengths, and m, a max, is bitwise the same
 * for every number of shares. */
int fa_decode_fwd(int dtype,
                  const void* Q, const void* K, const void* V,
                  void* O, float* l, float* m,
                  int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int64_t group,
                  const int* q_lens, const int* k_lens,
                  int64_t left, int64_t right,
                  float scale, void* workspace, size_t workspace_bytes,
                  void* hip_stream);

/* Workspace bytes fa_decode_fwd needs (0 is a valid answer: the keys are not split): the
 * fp32 partials of the key shares plus 256 B of slack.  It depends on the shape alone, not on
 * the lengths, the window or the device. */
size_t fa_decode_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv,
                               int64_t batch, int64_t group);

/* Decode attention over an fp8 KV cache: fa_decode_fwd with K and V stored as OCP e4m3fn bytes
 * (max 448, NaN at 0x7F / 0xFF, no infinity) plus one float32 scale per KV slab.  `dtype` stays
 * the type of Q and O (FA_DTYPE_BF16 or FA_DTYPE_F16); K8 is (Nk, d, batch) and V8
 * (Nk, dv, batch) bytes.  k_scale and v_scale are DEVICE pointers to `batch` floats; NULL means
 * 1.0.  With ks = k_scale[b], vs = v_scale[b] for KV slab b:
 *   s_ij = scale * ks * (q_i . k8_j);   m, l over these scores in natural-log units, as above;
 *   O = vs * sum_j P_ij v8_j.
 * Every e4m3fn value is exact in bf16 and fp16, so the arithmetic after the convert is
 * fa_decode_fwd's on the dequantised cache: ks is folded into the score scale and vs is applied
 * once where O is normalised; no element is multiplied by a scale.  The scales are device data
 * and are never read or validated on the host: they must be finite and > 0 (a non-positive ks
 * would turn the row max into a min; the results are then meaningless, but no access depends
 * on a scale).
 * Shapes, the `group` mapping, the device lengths and their clamping, the mask as a select,
 * the empty-row rule (O = +0, l = 0, m = -Inf), N * group <= 32, forward only, l and m float32
 * are fa_decode_fwd's.  Padding rows of K8 / V8 may hold any byte except the two NaN encodings
 * and change no output bit.
 * Checks, in order, all before any launch, and the empty cases: as fa_decode_fwd, the 32-bit
 * extents being a K8 / V8 slab below 2^31 bytes.  The cache is never copied: Nk % 16 != 0, or a
 * K8 / V8 pointer that is not 16-B aligned, selects an instantiation with single-byte loads.
 * The split over the keys, the merge order and the reproducibility are fa_decode_fwd's. */
int fa_decode_fp8_fwd(int dtype,
                      const void* Q, const void* K8, const void* V8,
                      const float* k_scale, const float* v_scale,
                      void* O, float* l, float* m,
                      int64_t N, int64_t Nk, int64_t d, int64_t dv, int64_t batch, int64_t group,
                      const int* q_lens, const int* k_lens,
                      int64_t left, int64_t right,
                      float scale, void* workspace, size_t workspace_bytes,
                      void* hip_stream);

/* Workspace bytes fa_decode_fp8_fwd needs: the same fp32 partials as fa_decode_fwd_workspace. */
size_t fa_decode_fp8_fwd_workspace(int dtype, int64_t N, int64_t Nk, int64_t d, int64_t dv,
                                   int64_t batch, int64_t group);

/* Decode attention over a PAGED KV cache: fa_decode_fwd with K and V kept as pools of fixed-size
 * pages and one page table per KV slab, as serving stacks store a cache.  In the library's
 * column-major convention K_pages is (page_size, d, num_pages), element (row t, feature f,
 * page p) at t + page_size * (f + d * p), and V_pages is (page_size, dv, num_pages): a page is a
 * small slab with keys contiguous per feature, exactly as a fa_decode_fwd slab.  block_table is
 * a DEVICE array (max_pages, batch) of int32: entry (j, b), at j + max_pages * b, is the
 * physical page that holds logical keys j * page_size .. (j + 1) * page_size - 1 of KV slab b.
 * The logical capacity cap = max_pages * page_size plays the role of Nk everywhere in
 * fa_decode_fwd's contract: the clamp of k_lens, off = nk - nq, windows >= cap are unbounded,
 * cap >= N is required.  Q, O, l, m, `group`, q_lens, k_lens, the mask as a select, the
 * empty-row rule (O = +0, l = 0, m = -Inf), N * group <= 32, bf16 / fp16 only, forward only are
 * fa_decode_fwd's.
 * The table is device data, never read or validated on the host.  The kernel reads entry
 * (j, b) only for j < ceil(nk_b / page_size), and clamps every entry it dereferences to
 * [0, num_pages) first: no access leaves the pools, whatever the table holds.  Entries at
 * j >= ceil(nk_b / page_size) may hold anything; pages that no read entry names may hold any
 * bit pattern, NaN included; rows of a slab's last page past nk_b may hold anything finite
 * (fa_decode_fwd's padding rule); none of this changes an output bit.  Two slabs may name the
 * same page (a shared prefix): pages are only read.
 * Checks, in order, all before any launch: null pointers (block_table is required);
 * DimensionMismatch (group, page_size, num_pages or max_pages below 1 included);
 * FA_ERR_UNSUPPORTED for head dims, cap < N, N * group > 32, dtype, page_size % 8 != 0, K_pages
 * or V_pages not 16-B aligned; the kernels' 32-bit extents (one page below 2^31 bytes, cap below
 * 2^31; the pools have no size limit, page bases are 64-bit); the workspace.  N == 0 or
 * batch == 0 is a no-op that dereferences nothing.
 * The cache is never copied or gathered.  page_size % 64 == 0 runs the instantiation that builds
 * one buffer descriptor per key tile from its table entry; every other multiple of 8 the one
 * whose lanes look up the page of each 16-B chunk of 8 keys.  The split over the keys, the
 * merge order and the reproducibility are fa_decode_fwd's, and the outputs do not depend on
 * where in the pools the pages lie. */
int fa_decode_paged_fwd(int dtype,
                        const void* Q, const void* K_pages, const void* V_pages,
                        const int* block_table,
                        void* O, float* l, float* m,
                        int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                        int64_t page_size, int64_t num_pages, int64_t max_pages,
                        const int* q_lens, const int* k_lens,
                        int64_t left, int64_t right,
                        float scale, void* workspace, size_t workspace_bytes,
                        void* hip_stream);

/* Workspace bytes fa_decode_paged_fwd needs: fa_decode_fwd_workspace at Nk = max_pages *
 * page_size (the fp32 partials of the key shares only). */
size_t fa_decode_paged_fwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch,
                                     int64_t group, int64_t page_size, int64_t max_pages);

/* Decode attention over a PAGED fp8 KV cache: fa_decode_paged_fwd's cache layout with
 * fa_decode_fp8_fwd's element type, as a serving stack that keeps an fp8 cache stores it.
 * K8_pages is (page_size, d, num_pages) and V8_pages (page_size, dv, num_pages) BYTES, OCP e4m3fn
 * (max 448, NaN at 0x7F / 0xFF, no infinity), element (row t, feature f, page p) at
 * t + page_size * (f + d * p); block_table is a DEVICE array (max_pages, batch) of int32 exactly
 * as for fa_decode_paged_fwd, and cap = max_pages * page_size stands wherever fa_decode_fwd has
 * Nk.  k_scale and v_scale are DEVICE pointers to `batch` floats, one per KV slab (not per page),
 * NULL meaning 1.0, finite and > 0, never read or validated on the host: s_ij = scale * ks *
 * (q_i . k8_j), O = vs * sum_j P_ij v8_j; ks is folded into the score scale and vs is applied
 * once where O is normalised; no element is multiplied by a scale.  Two slabs may name the same
 * page (a shared prefix; pages are only read); giving such slabs equal scales is the caller's
 * business: each slab reads the page's bytes under its own scales.
 * `dtype` is the type of Q and O (FA_DTYPE_BF16 or FA_DTYPE_F16).  Q, O, l, m, `group`, q_lens,
 * k_lens, the mask as a select, the empty-row rule (O = +0, l = 0, m = -Inf), N * group <= 32 and
 * forward only are fa_decode_fwd's.
 * The table rules are fa_decode_paged_fwd's: entry (j, b) is read only for
 * j < ceil(nk_b / page_size) and every entry is clamped to [0, num_pages) before it forms an
 * address, so no access leaves the pools whatever the table holds.  Entries past that, and pages
 * that no read entry names, may hold any byte, the two NaN encodings included.  Rows of a slab's
 * last page past nk_b may hold any byte except 0x7F and 0xFF (fa_decode_fp8_fwd's padding rule).
 * None of this changes an output bit.
 * Checks, in order, all before any launch: null pointers (block_table is required; the scales
 * may be NULL); DimensionMismatch (group, page_size, num_pages or max_pages below 1 included);
 * FA_ERR_UNSUPPORTED for head dims, cap < N, N * group > 32, dtype, page_size % 16 != 0 (a 16-B
 * chunk of 16 keys must lie in one page), K8_pages or V8_pages not 16-B aligned; the kernels'
 * 32-bit extents (one page below 2^31 bytes, cap below 2^31; the pools have no size limit); the
 * workspace.  N == 0 or batch == 0 is a no-op that dereferences nothing.
 * The cache is never copied, gathered or widened.  page_size % 64 == 0 runs the instantiation
 * that builds one buffer descriptor per key tile from its table entry; every other multiple of
 * 16 the one whose lanes look up the page of each 16-B chunk of 16 keys.  The split over the
 * keys, the merge order and the reproducibility are fa_decode_fwd's; the outputs do not depend
 * on where in the pools the pages lie and are bitwise those of fa_decode_fp8_fwd on the gathered
 * cache. */
int fa_decode_paged_fp8_fwd(int dtype,
                            const void* Q, const void* K8_pages, const void* V8_pages,
                            const float* k_scale, const float* v_scale,
                            const int* block_table,
                            void* O, float* l, float* m,
                            int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                            int64_t page_size, int64_t num_pages, int64_t max_pages,
                            const int* q_lens, const int* k_lens,
                            int64_t left, int64_t right,
                            float scale, void* workspace, size_t workspace_bytes,
                            void* hip_stream);

/* Workspace bytes fa_decode_paged_fp8_fwd needs: fa_decode_fwd_workspace at Nk = max_pages *
 * page_size (the fp32 partials of the key shares only). */
size_t fa_decode_paged_fp8_fwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch,
                                         int64_t group, int64_t page_size, int64_t max_pages);

/* Chunked PREFILL attention over a paged KV cache: fa_decode_paged_fwd without its row limit, for
 * a few hundred or thousand new tokens appended to a cached context (k_lens = context + N), a
 * prefix-cache hit followed by the rest of the prompt, or tree decoding with wide groups.  Every
 * argument, the layouts of Q, O, l, m, K_pages, V_pages and block_table, `group` (query slab bq
 * reads KV slab bq / group), q_lens, k_lens (NULL: full), the mask (with off = nk - nq, query
 * i < nq sees keys i + off - left <= j <= i + off + right, 0 <= j < nk; a negative side is
 * unbounded), the empty-row rule (rows i >= nq and key-less queries: O = +0, l = 0, m = -Inf),
 * cap = max_pages * page_size in the role of Nk, and the table rules (entry (j, b) read only for
 * j < ceil(nk_b / page_size), clamped to [0, num_pages) before it forms an address; entries past
 * that and pages no read entry names may hold anything; rows of a slab's last page past nk_b and
 * padding rows of Q anything finite; shared pages allowed) are fa_decode_paged_fwd's.  N is any
 * value >= 1 with cap >= N and group any value >= 1: N * group <= 32 is accepted too.  bf16 /
 * fp16, d and dv up to 128, page_size any positive multiple of 8, forward only.
 * A contiguous (Nk, d, batch) cache with Nk % 8 == 0 is the pool with page_size = Nk,
 * num_pages = batch, max_pages = 1 and block_table[0, b] = b: grouped-query prefill over a plain
 * cache, through the same kernels, without `group` copies of K and V.
 * Checks, in order, all before any launch: null pointers (block_table is required);
 * DimensionMismatch (group, page_size, num_pages or max_pages below 1 included);
 * FA_ERR_UNSUPPORTED for head dims, cap < N, dtype, page_size % 8 != 0, K_pages or V_pages not
 * 16-B aligned; the kernels' 32-bit extents (one page below 2^31 bytes, cap below 2^31, the
 * N * group rows of a KV slab times max(d, dv) below 2^30 elements; the pools have no size
 * limit); the workspace.  N == 0 or batch == 0 is a no-op that dereferences nothing.
 * The cache is never copied, gathered or repeated.  The rows of a KV slab, position-major, are cut
 * into blocks of 128 that share each key tile through LDS; page_size % 64 == 0 runs the
 * instantiation that stages a tile by LDS-DMA through one descriptor per tile, every other
 * multiple of 8 the one whose threads look up the page of each 16-B chunk.  Small grids split the
 * keys (workspace: fp32 partials, merged in split order): no atomics, all three outputs bitwise
 * reproducible and independent of where the pages lie, m the same bits for every split count. */
int fa_prefill_paged_fwd(int dtype,
                         const void* Q, const void* K_pages, const void* V_pages,
                         const int* block_table,
                         void* O, float* l, float* m,
                         int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                         int64_t page_size, int64_t num_pages, int64_t max_pages,
                         const int* q_lens, const int* k_lens,
                         int64_t left, int64_t right,
                         float scale, void* workspace, size_t workspace_bytes,
                         void* hip_stream);

/* Workspace bytes fa_prefill_paged_fwd needs: 0 unless the keys are split, then the fp32 partials
 * [nsplit][batch * group][N][dv + 2] (+ 256). */
size_t fa_prefill_paged_fwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch,
                                      int64_t group, int64_t page_size, int64_t max_pages);

/* Chunked PREFILL attention over a PAGED fp8 KV cache: fa_decode_paged_fp8_fwd without its row
 * limit, for a serving stack that keeps its cache as fp8 byte pages and runs a chunked prefill, a
 * prefix-cache hit followed by the rest of the prompt, or tree decoding with N * group > 32.  The
 * argument list is fa_decode_paged_fp8_fwd's and the contract is the union of two:
 * from fa_prefill_paged_fwd, any N >= 1 and group >= 1 (N * group <= 32 included), the row order,
 * the mask with off = nk - nq, the empty-row rule (O = +0, l = 0, m = -Inf by select),
 * cap = max_pages * page_size in the role of Nk, the table rules (entry (j, b) read only for
 * j < ceil(nk_b / page_size), every entry clamped to [0, num_pages) before it forms an address),
 * shared pages, forward only, bf16 / fp16 Q and O (`dtype`), d and dv up to 128;
 * from fa_decode_paged_fp8_fwd, K8_pages (page_size, d, num_pages) and V8_pages (page_size, dv,
 * num_pages) of OCP e4m3fn BYTES, element (row t, feature f, page p) at t + page_size * (f + d * p);
 * k_scale and v_scale DEVICE pointers to `batch` floats, one per KV slab, NULL meaning 1.0, finite
 * and > 0, never read on the host; s_ij = scale * ks * (q_i . k8_j), O = vs * sum_j P_ij v8_j, ks
 * folded into the score scale, vs applied once where O is normalised, no element multiplied by a
 * scale; and the padding rule: rows of a slab's last page past nk_b may hold any byte except 0x7F
 * and 0xFF, pages that no read entry names and entries past ceil(nk_b / page_size) anything.
 * A contiguous (Nk, d, batch) byte cache with Nk % 16 == 0 is the pool with page_size = Nk,
 * num_pages = batch, max_pages = 1 and block_table[0, b] = b.
 * Checks, in order, all before any launch: null pointers (block_table is required; the scales
 * may be NULL); DimensionMismatch (group, page_size, num_pages or max_pages below 1 included);
 * FA_ERR_UNSUPPORTED for head dims, cap < N, dtype, page_size % 16 != 0 (a 16-B chunk of 16 keys
 * must lie in one page), K8_pages or V8_pages not 16-B aligned; the kernels' 32-bit extents (one
 * page below 2^31 bytes, cap below 2^31, the N * group rows of a KV slab times max(d, dv) below
 * 2^30 elements; the pools have no size limit); the workspace.  N == 0 or batch == 0 is a no-op
 * that dereferences nothing.
 * The cache is never copied, gathered or widened: the bytes are staged in LDS as bytes and
 * converted (exactly) in registers before the MFMAs.  The rows of a KV slab, position-major, are
 * cut into blocks of 128 that share each key tile through LDS; page_size % 64 == 0 runs the
 * instantiation that stages a tile by LDS-DMA through one descriptor per tile, every other
 * multiple of 16 the one whose threads look up the page of each 16-B chunk of 16 keys.  Small
 * grids split the keys (workspace: fp32 partials, merged in split order): no atomics, all three
 * outputs bitwise reproducible and independent of where the pages lie, m the same bits for every
 * split count. */
int fa_prefill_paged_fp8_fwd(int dtype,
                             const void* Q, const void* K8_pages, const void* V8_pages,
                             const float* k_scale, const float* v_scale,
                             const int* block_table,
                             void* O, float* l, float* m,
                             int64_t N, int64_t d, int64_t dv, int64_t batch, int64_t group,
                             int64_t page_size, int64_t num_pages, int64_t max_pages,
                             const int* q_lens, const int* k_lens,
                             int64_t left, int64_t right,
                             float scale, void* workspace, size_t workspace_bytes,
                             void* hip_stream);

/* Workspace bytes fa_prefill_paged_fp8_fwd needs: 0 unless the keys are split, then the fp32
 * partials [nsplit][batch * group][N][dv + 2] (+ 256). */
size_t fa_prefill_paged_fp8_fwd_workspace(int dtype, int64_t N, int64_t d, int64_t dv, int64_t batch,
                                          int64_t group, int64_t page_size, int64_t max_pages);

/* WRITE new K / V rows into a PAGED 16-bit KV cache: the first half of a decode step ("put this
 * token's K and V into their pages, then attend") and of a chunked prefill.  The arguments mean
 * what they mean for fa_prefill_paged_fwd, with group = 1 on the KV side: the append and the
 * attention call that follows it take the same (q_lens, k_lens); k_lens is the length AFTER the
 * append.  K_new (N, d, batch), V_new (N, dv, batch); K_pages (page_size, d, num_pages), V_pages
 * (page_size, dv, num_pages), element (row t, feature f, page p) at t + page_size * (f + d * p);
 * block_table (max_pages, batch) int32 on the device.
 * Per slab b: nq = clamp(q_lens[b], 0, N), nk = clamp(k_lens[b], 0, cap), cap = max_pages *
 * page_size, clamped on the device and never read on the host (NULL = N, cap).  New row i < nq is
 * the key at logical position j = nk - nq + i, the position the prefill's mask gives query i, and
 * goes to row j % page_size of page clamp(block_table[j / page_size, b], 0, num_pages - 1), for
 * every feature of K and of V.  Rows i >= nq and rows with j < 0 (nk < nq) are not written.  A table
 * entry is read only for a page that the written range [max(nk - nq, 0), nk) touches.
 * Guarantees: every written element is bitwise the source element; every other byte of both pools
 * is bitwise unchanged; no pool byte is read (no read-modify-write of neighbours); no access
 * leaves the pools or the (N, ., batch) sources, whatever the table and the lengths hold; each
 * destination element is written once, so the result is bitwise reproducible; no atomics, no
 * workspace, no allocation, no synchronisation.
 * The caller's business: the pages in one slab's written range must not be named by another
 * slab's written range in the same call (copy-on-write of shared prefixes happens outside the
 * library).  If they are, the values in those pages are unspecified; safety still holds.
 * Checks, in order, all before any launch: null pointers (K_new, V_new, both pools and block_table
 * are required, the lengths may be NULL); DimensionMismatch (d, dv, page_size, num_pages or
 * max_pages below 1, negative N or batch); FA_ERR_UNSUPPORTED for head dims above
 * fa_max_head_dim(), cap < N, a dtype other than bf16 / fp16, page_size % 8 != 0, pools that are
 * not 16-B aligned; the 32-bit extents (one page below 2^31 bytes, cap below 2^31, one source
 * slab below 2^31 bytes).  N == 0 or batch == 0 is a no-op that dereferences nothing.  K_new and
 * V_new may start at any element-aligned address.
 * The work is split by destination: a workgroup owns (slab, touched page, feature range), looks
 * its page up once, stages the source runs through LDS and stores 16-B destination-aligned
 * chunks, the ragged head and tail as narrower stores of exactly the owned elements.  N == 1 (the
 * decode step) runs one thread per feature of K and of V, several slabs per workgroup. */
int fa_kv_append_paged(int dtype,
                       const void* K_new, const void* V_new,
                       void* K_pages, void* V_pages,
                       const int* block_table,
                       int64_t N, int64_t d, int64_t dv, int64_t batch,
                       int64_t page_size, int64_t num_pages, int64_t max_pages,
                       const int* q_lens, const int* k_lens,
                       void* hip_stream);

/* fa_kv_append_paged into pools of OCP e4m3fn BYTES: K8_pages (page_size, d, num_pages), V8_pages
 * (page_size, dv, num_pages), as fa_decode_paged_fp8_fwd and fa_prefill_paged_fp8_fwd read them.
 * `dtype` is the type of K_new and V_new (bf16 / fp16).  k_scale, v_scale: DEVICE pointers to
 * `batch` floats, one per slab, NULL meaning 1.0, finite and > 0, never read on the host.  The
 * written byte is e4m3fn_rne(clamp(float(x) / s_b, -448, 448)): an IEEE fp32 division (not a
 * multiplication by a reciprocal), round-to-nearest-even onto the e4m3fn grid, subnormals and the
 * sign of zero included: bit for bit what the float32 expression
 * (x.float() / s).clamp(-448, 448) converted to float8_e4m3fn gives on the host.  Sources are
 * finite or +-Inf (Inf saturates to +-448); NaN sources are outside the contract.  Everything else
 * is fa_kv_append_paged's, with page_size % 16 != 0 refused, as the fp8 readers refuse it. */
int fa_kv_append_paged_fp8(int dtype,
                           const void* K_new, const void* V_new,
                           void* K8_pages, void* V8_pages,
                           const float* k_scale, const float* v_scale,
                           const int* block_table,
                           int64_t N, int64_t d, int64_t dv, int64_t batch,
                           int64_t page_size, int64_t num_pages, int64_t max_pages,
                           const int* q_lens, const int* k_lens,
                           void* hip_stream);

/* A contiguous 16-bit cache as e4m3fn bytes with one scale per slab: K (Nk, d, batch), V (Nk, dv,
 * batch) of `dtype` (bf16 / fp16) to K8, V8 (bytes, the same shapes) and k_scale, v_scale (`batch`
 * floats each, device).  Per slab amax = max |x| (exact, order-free), s = amax > 0 ? amax / 448 :
 * 1, and every byte is fa_kv_append_paged_fp8's expression with that s.  Two kernels: the first
 * writes the maxima of fixed spans of each slab to the workspace, the second reduces its slab's
 * maxima, writes the scale and converts.  No atomics, bitwise reproducible.  Sources finite.
 * Checks, in order: null pointers, DimensionMismatch (d or dv below 1, negative Nk or batch),
 * FA_ERR_UNSUPPORTED for a dtype other than bf16 / fp16 and for a slab of 2^31 bytes or more,
 * FA_ERR_WORKSPACE.  Nk == 0 or batch == 0 is a no-op that dereferences nothing (no scale is
 * written). */
int fa_kv_quantize_fp8(int dtype, const void* K, const void* V,
                       void* K8, void* V8, float* k_scale, float* v_scale,
                       int64_t Nk, int64_t d, int64_t dv, int64_t batch,
                       void* workspace, size_t workspace_bytes, void* hip_stream);

/* Workspace bytes fa_kv_quantize_fp8 needs: the spans' maxima, [2][batch][parts] floats (+ 256);
 * 0 for a shape it refuses or for which it does nothing. */
size_t fa_kv_quantize_fp8_workspace(int dtype, int64_t Nk, int64_t d, int64_t dv, int64_t batch);

/* Standalone fused softmax, replaces
 *   fused_softmax!(P, S; dims)   reference src/fused_softmax.jl:1-41
 * (device versions src/cuda/fused_softmax.jl:11-314).  S, P: (M, N, batch)
 * column-major, same dtype; dims = 1 normalises each column S[:, j, b]
 * (M contiguous elements), dims = 2 each row S[i, :, b].  P may equal S
 * (in place, fused_softmax!(S)).  A vector is (M, 1, 1) with dims = 1.
 * Computed in fp32; an all -Inf or NaN-containing vector gives NaN, as the
 * reference's arithmetic does.  batch == 0 is a no-op; M or N == 0 is
 * rejected (a reduction over an empty dimension). */
size_t fa_softmax_workspace(int64_t M, int64_t N, int64_t batch, int dims);
int fa_softmax(int dtype, const void* S, void* P, int64_t M, int64_t N, int64_t batch, int dims,
               void* workspace, size_t workspace_bytes, void* hip_stream);

/* Thread-local description of the last error on this host thread ("" if none). */
const char* fa_last_error(void);

/* FA_HIP_ABI_VERSION of the loaded library. */
int fa_abi_version(void);

/* Largest d (and dv) the kernels accept. */
int fa_max_head_dim(void);

#ifdef __cplusplus
}
#endif

#endif /* FA_HIP_H */
