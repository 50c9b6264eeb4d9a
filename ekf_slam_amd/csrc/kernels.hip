// gfx950 (MI355X / CDNA4) kernels of the EKF-SLAM update engine.
//
// The path as the reference writes it is HBM- or latency-bound (AI of the rank-2 downdate is 0.25 flop/B in f64), so the
// rules that matter are: 16-byte-per-lane coalesced accesses on whole 64-lane wavefronts, many independent loads in
// flight per lane, >> 256 workgroups per launch, nothing re-read from HBM that can be kept in registers, no host
// synchronisation between launches.  Two pieces ARE GEMM-shaped and run on the f64 matrix cores, bit-identical to
// their scalar fma formulation: the deferred rank-2m flush (k_flush_mfma) and the predict panel (k_predict_mfma).
//
// Reference expressions realised (file:line in the reference tree):
//   k_predict    P = F*P*F' + Q, x = f(x,u), wrapTo360          EKF_SLAM.m:40-51,56-65
//   k_predict_model  the same step with true Jacobians, m per launch  (no counterpart: EKF_SLAM.m:58-60 is its model 1's f)
//   k_append     state/covariance growth                         EKF_SLAM.m:67-98 (append.m:1-27)
//   k_gather     z_k, H_k, phi_k, K, x += K nu                   EKF_SLAM.m:125-144
//   k_downdate*  P = (I - K H_k) P  ==  P - K (H_k P)            EKF_SLAM.m:145
//   k_flush_*    the same for m deferred corrections in one pass  EKF_SLAM.m:145 (x m)
//   k_associate  per-landmark phi_k, Mahalanobis + signature     Correspondence.m:49-87
#include "kernels.h"

#include <algorithm>
#include <atomic>
#include <climits>
#include <cstdio>
#include <type_traits>

#include "device_math.h"
#include "flush32_mfma.h"     // kBlock, ring_slot, k_flush_mfma32
#include "flush32_pipe.h"     // k_flush_strip32, the strip work list
#include "flush32_split.h"    // k_split_pairs, k_flush_split3
#include "flush64_mfma.h"     // k_flush_mfma

// The kernels, by family (each header is a fragment of THIS translation unit, not a stand-alone interface):
namespace {

#include "tile_access.h"      // canonical element access, rank2_apply
#include "lane_ops.h"         // values between the lanes of a wavefront: lane_bcast, lane_gather, lane_xor1
#include "predict.h"          // k_predict, k_predict_mfma and the shared 3x3 part
#include "predict_model.h"    // k_predict_model: a chain of motion steps through the models of ekfm::motion_eval, one launch
#include "assoc_winners.h"    // association order, the self-validating winner entries
#include "append.h"           // k_append
#include "append_model.h"     // k_append_model: a scan's landmarks from range-bearing / relative-position fixes, one launch
#include "join_map.h"         // k_join_state, k_join_rows: a local map joined into the map (a composition of the two above)
#include "extract_map.h"      // k_extract_state, k_extract_rows: part of a map taken out into another handle
#include "solve_small.h"      // the 5x5 solve, entry by entry
#include "rowpanel.h"         // PanelView, k_rowpanel, k_rowpanel_next, k_rowpanel_base
#include "pair_column.h"      // what every producer of a pair (K, G) does per column: the pair's slot, x', strip', the diagonal blocks
#include "gather.h"           // k_gather
#include "downdate.h"         // k_downdate, k_downdate_w
#include "associate.h"        // k_associate, k_assoc_merge
#include "state_io.h"         // dense <-> tiled, block reads, low-rank load, digest
#include "compact.h"          // landmark removal: k_compact_tiles, k_compact_state
#include "transform_map.h"    // k_transform_state, k_transform_tiles: the whole map moved into another frame, in place (extract_map.h's and join_map.h's blocks, downdate.h's Lane16)
#include "constrain.h"        // a constraint between two landmarks: k_constrain_probe, k_gather_constrain
#include "linear_obs.h"       // a linear observation as an update-step: k_gather_linear, k_linear_probe
#include "model_obs.h"        // ... through a range / bearing / relative-position model evaluated at the live x: k_gather_model, k_model_probe
#include "model_assigned.h"   // ... with the landmark read from a scan's assignment on the device: k_gather_model_assigned
#include "model_iter.h"       // ... relinearised on lane 0 (the iterated EKF update): k_gather_model_iter, k_model_iter_probe
#include "associate_model.h" // a scan against the whole map under the models' conventions: k_assoc_model, k_assoc_model_reduce
#include "assign_model.h"    // ... and assigned to it one-to-one: k_assign_candidates, k_assign_select, k_assign_solve
#include "joint.h"            // a scan's pairings judged jointly, a hypothesis per workgroup: k_joint_innovation
#include "joint_search.h"     // ... and searched for the jointly compatible hypothesis, level by level: k_joint_search_prepare / _extend / _select
#include "joint_update.h"     // ... and applied as one joint update: k_joint_factor, k_gather_joint
#include "joint_iter.h"       // ... relinearised: k_joint_factor_iter
#include "merge_pass.h"       // the fused downdate-and-compact pass of a batch of merges: k_merge_pass
#include "nearest.h"          // the candidate search in front of a merge: k_nearest
#include "factor_map.h"       // the Cholesky factorisation of P in a scratch store: k_factor_load / _rhs / _diag / _panel / _trail / _finish
#include "map_blocks.h"       // what the calls on P as a matrix share: chunk_k, tile_mac, segment_of, chunk_tree_sums
#include "sample_map.h"       // ... and the draws x + C xi behind it: k_factor_apply, k_factor_sample
#include "solve_map.h"        // ... and the solves C^-1 B, P^-1 B: k_solve_invert, k_solve_forward, k_solve_tail, k_solve_backward
#include "multiply_map.h"     // the plain product P B on the handle's own tile store, no factor: k_multiply_tiles, k_multiply_sum, k_multiply_robot
#include "dense_obs.h"        // ... and a linear observation with a dense H behind it: k_dense_gram, k_dense_factor, k_gather_dense

}  // namespace

// The launchers kernels.h declares, by family, in its order (fragments of this translation unit too):
#include "launch/dispatch.h"      // a run-time storage type / flag -> a template argument; clamp_grid
#include "launch/steps.h"         // predict, append, gather, row-panels, association
#include "launch/pass_select.h"   // which pass instance runs: a pure function, no HIP
#include "launch/passes.h"        // launch_downdate, the row copies behind an asynchronous pass
#include "launch/edits.h"         // compact, extract, transform, merge pass, constrain, linear and model observations, joint innovation, joint search and joint update, nearest
#include "launch/map_sizes.h"     // the sizing arithmetic of the calls that treat P as a matrix: host code, no HIP
#include "launch/map_algebra.h"   // the factorisation, the draws and the solves behind it, the plain product, the dense observation
#include "launch/state_io.h"      // dense <-> tiled, block reads, low-rank load, digest
