/* Density clustering (DBSCAN) of facial IDs on the device (fid_cluster.hip): which unlabelled faces are the
 * same person.  Part of the C ABI of libfv_hotpath; the declarations live here and not in include/fv_hotpath.h for the reason
 * DESIGN.md section 30 gives for tile_merge.h (the stream-order table has a row per function declared under include/).  Additive:
 * fv_abi_version() is unchanged. */
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/fv_hotpath.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FV_FID_CLUSTER_MAX_N 65536 /* rows one fv_fid_cluster call takes (a bit matrix of n * n / 8 bytes: 512 MiB there) */

/* Bytes of device workspace fv_fid_cluster needs for n rows: 0 for n outside 1..FV_FID_CLUSTER_MAX_N, non-decreasing in n. */
size_t fv_fid_cluster_workspace_bytes(int n);

/* ids [n][64] float32, 16-byte aligned.
 *
 * Distance.   D(i, r) is fv_fid_match's distance: the square root of the fp64 sum, in dimension order 0..63, of the squared fp64
 *             differences (no FMA contraction: -ffp-contract=off).  So D(i, r) == D(r, i) bit for bit.
 * Neighbours. r is a neighbour of i when D(i, r) <= eps.  A row is its own neighbour when D(i, i) = 0 <= eps.  A NaN distance is
 *             not a neighbour, so a row that holds a NaN or an inf has no neighbours at all (not even itself).
 * n_nbr[i]    the number of neighbours of i.
 * core[i]     1 when n_nbr[i] >= min_pts, else 0 (scikit-learn's rule: the point itself counts).
 * Clusters.   A cluster is a connected component of the graph on the core rows whose edges are the neighbour pairs.
 * Numbering.  Clusters are numbered 0..C-1 by ascending smallest member core index.  n_clusters[0] = C.
 * Borders.    A non-core row with at least one core neighbour is a border row.  It joins the cluster of its nearest core
 *             neighbour: the minimum of (D, r) under min_less (block_ops.h), so the nearer core wins and the lower index wins among
 *             equal distances.  (scikit-learn gives a border row to whichever cluster reaches it first in row order.)
 * Noise.      Every other non-core row.
 * labels[i]   the cluster number, or -1 for noise.
 * via[i]      i for a core row, the claiming core row for a border row, -1 for noise.
 *
 * Determinism.  The five outputs (labels, via, n_nbr [n] int32, core [n] uint8, n_clusters [1] int32) are a function of
 * (ids, n, eps, min_pts) only: not of launch geometry, of timing, or of what workspace and outputs held on entry (the workspace
 * contract of DESIGN.md section 27).  Integer atomics (compare-and-swap and minimum on the union-find parents) are used only where
 * the final value does not depend on their order; no float atomics.
 *
 * workspace: device memory of at least fv_fid_cluster_workspace_bytes(n) bytes, 8-byte aligned.
 *
 * FV_ERR_INVALID with nothing enqueued and the outputs untouched for: a NULL pointer, n outside 1..FV_FID_CLUSTER_MAX_N, eps not
 * finite or < 0, min_pts < 1, ids not 16-byte aligned, workspace not 8-byte aligned.
 *
 * Stream order: seven launches on the context's stream; nothing waits for the stream (the calls that do are fv_fid_pair_dists and
 * fv_fid_mine_negatives, which upload a table; this one is not among them: the components are found by a lock-free union-find in
 * one launch, with no convergence flag for the host to read). */
int fv_fid_cluster(fv_ctx* ctx, const float* ids, int n, double eps, int min_pts, void* workspace, int32_t* labels, int32_t* via,
                   int32_t* n_nbr, uint8_t* core, int32_t* n_clusters);

#ifdef __cplusplus
}
#endif
