/*
 * mpgpu.h — C ABI of libmpgpu.so, the MI355X (gfx950) hot path of
 * congkaishen/MotionPlanning.
 *
 * The reference is pure Julia; these entry points are what its planner calls
 * through `ccall` (binding shown in INTEGRATION.md, wrapper in julia/MPGPU.jl).
 * Every entry point cites the reference interface it replaces.
 *
 * Conventions
 *  - All functions return an int status: MP_OK (0) or an MP_ERR_* code; the
 *    message is available from mp_last_error(ctx).  This mirrors the
 *    reference's `error(...)` validation (OptimalControl/MPPI/src/setup.jl:19-38).
 *  - Arrays are dense, C row-major.  Shapes are written in C order; the
 *    equivalent Julia column-major shape is the reverse, e.g. noise
 *    [S][K][H][2] here == Array{Float64}(2, H, K, S) in Julia.
 *  - Functions without the _dev suffix take HOST pointers, are synchronous,
 *    and return after all results have been copied back (Julia arrays are
 *    rooted for the duration of the ccall).  _dev variants take DEVICE
 *    pointers, enqueue on the context's stream and do not synchronise.
 *  - A context owns one HIP device, one stream and cached device workspaces.
 *    It is not thread-safe; use one context per GPU / thread.
 *  - Precision: Float64 throughout, like the reference.
 */
#ifndef MPGPU_H
#define MPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPGPU_VERSION "0.1.0"

#define MP_OK 0
#define MP_ERR_INVALID 1   /* bad argument (shape, NULL, range)            */
#define MP_ERR_HIP 2       /* HIP runtime error                            */
#define MP_ERR_NOMEM 3     /* device allocation failed                     */
#define MP_ERR_NUMERIC 4   /* NaN / domain flag raised (outputs written)   */
#define MP_ERR_UNSUPPORTED 5

typedef struct mp_ctx mp_ctx;

/* ------------------------------------------------------------- context */
int mp_ctx_create(int device, mp_ctx** out);
int mp_ctx_destroy(mp_ctx* ctx);
const char* mp_last_error(mp_ctx* ctx);
const char* mp_version(void);
int mp_device_count(int* n);
/* Synchronise the context stream and its side stream (after _dev calls). */
int mp_ctx_synchronize(mp_ctx* ctx);
/* Order the context stream after all side-stream work enqueued so far (the deferred
 * MPPI final rollouts, mp_mppi_params.final_stream = 1): consumers of traj_out /
 * cost_out / feasible_out on the context stream call this first. */
int mp_ctx_join(mp_ctx* ctx);
/* The hipStream_t the context launches on (for HIP-event timing). */
void* mp_ctx_stream(mp_ctx* ctx);
/* Kernel timing: when enabled, every launch of the dominant kernel of a call
 * (mppi_plan_kernel, ...) is bracketed by HIP events on the context stream;
 * mp_ctx_kernel_ms synchronises, returns the summed milliseconds and launch
 * count since the last query, and resets them. */
int mp_ctx_kernel_timing(mp_ctx* ctx, int enable);
int mp_ctx_kernel_ms(mp_ctx* ctx, double* ms_sum, int32_t* count);
/* Device workspaces.  A context caches its scratch buffers across calls (they only grow, with
 * 25 % headroom).  mp_ctx_trim synchronises and frees every cached buffer larger than
 * keep_bytes (0: all of them); later calls re-allocate what they need.
 * mp_ctx_set_workspace_limit caps any single buffer (0: no cap).  Optional speed-up buffers
 * (mp_ilqr_solve's all-trials-at-once line-search slots, which are also skipped when they
 * would take more than half of the free device memory) fall back to a smaller layout with
 * identical results; a call that cannot run within the cap returns MP_ERR_NOMEM. */
int mp_ctx_trim(mp_ctx* ctx, size_t keep_bytes);
int mp_ctx_set_workspace_limit(mp_ctx* ctx, size_t bytes);

/* ---------------------------------------------------------------- MPPI */
#define MP_NX 7 /* [x, y, v, r, psi, ux, sa]  vehicledynamics.jl:20-26 */
#define MP_NU 2 /* [sr, ax]                    vehicledynamics.jl:27-28 */

#define MP_NOISE_EXTERNAL 0 /* z ~ N(0,I) supplied by the caller (parity mode) */
#define MP_NOISE_PHILOX 1   /* Philox4x32-10 + Box–Muller on device            */

/* Planner settings; fields mirror MPPISetting (OptimalControl/MPPI/src/types.jl:10-31). */
typedef struct mp_mppi_params {
  int32_t K;                 /* SamplingNumber                                  */
  int32_t H;                 /* N, horizon steps                                */
  int32_t feasibility_count; /* FeasibilityCount (default 1300); >= K disables  */
  int32_t n_obs;             /* circles per scene ([x, y, R] each)              */
  double dt;                 /* T / N                                           */
  double lambda;             /* λ                                               */
  double sigma[4];           /* Σ, row-major 2x2                                */
  double XL[MP_NX], XU[MP_NX];
  double CL[MP_NU], CU[MP_NU];
  double slack_penalty;      /* SlackPenalty (1e5)                              */
  double obs_penalty;        /* 100*712.5 (MPPIUtils.jl:127); DWA: 10000*712.5  */
  int32_t grid_nx, grid_ny;  /* occupancy grid (build extension), 0 = none: after */
                             /*   the circles, a state with fx = (x - grid_x0) / */
                             /*   grid_dx in [0, nx), fy likewise in [0, ny) and */
                             /*   grid[(int)fy][(int)fx] != 0 is infeasible and  */
                             /*   costs one more obs_penalty; off the grid: free */
  double grid_x0, grid_y0, grid_dx, grid_dy;
  int32_t noise_mode;        /* MP_NOISE_*                                      */
  int32_t ctrl_cost;         /* 1: λ·u_nomᵀΣ⁻¹(u−u_nom) term (MPPIUtils.jl:45)  */
  uint64_t seed;             /* Philox key                                      */
  uint64_t offset;           /* Philox counter word (advance per solve)         */
  int32_t scene_base;        /* global index of this call's scene 0 (Philox     */
                             /*   counter word): a rank planning scenes [a,b)   */
                             /*   of a sharded batch passes a, so every scene   */
                             /*   draws the same stream at any world size       */
  int32_t final_stream;      /* 0: the final TrajectoryRollout(MPPICtrl) runs   */
                             /*   at the end of the plan kernel.  1: it runs on */
                             /*   the context's side stream from a snapshot of  */
                             /*   its inputs, overlapping the next call's       */
                             /*   rollouts (see mp_mppi_plan_dev)               */
  int32_t calls_in_flight;   /* 0 / 1: the call has the device to itself.  n > 1:*/
                             /*   the caller keeps n independent calls in       */
                             /*   flight on n contexts of this device (see      */
                             /*   INTEGRATION.md); the launch then takes the    */
                             /*   layout whose waves share the CUs with the     */
                             /*   other calls' (one rollout per lane).  Same    */
                             /*   rollouts bit for bit either way; MPPICtrl     */
                             /*   within the combine tolerance (the weighted    */
                             /*   sum's partition may differ)                   */
} mp_mppi_params;

/*
 * mp_mppi_plan — one MPPIPlan(mppi) per scene (OptimalControl/MPPI/src/MPPIUtils.jl:169-203),
 * S independent scenes per call.
 *
 * in : X0[S][7]       MPPI.s.X0 (ShiftInitialCondition, MPPIUtils.jl:24-27)
 *      goal[S][2]     MPPI.s.goal
 *      U_nom[S][H][2] MPPI.s.NominalControl (defineMPPINominalControl!, setup.jl:70-80)
 *      obstacles[S][n_obs][3]  MPPI.s.obstacle_list (defineMPPIobs!, setup.jl:61-64), may be NULL if n_obs == 0
 *      grid[S][ny][nx] uint8 occupancy (1 = occupied), NULL if grid_nx == 0
 *      noise[S][K][H][2]  standard normals z (MP_NOISE_EXTERNAL), else NULL;
 *                     control = clamp(U_nom + L z, CL, CU), L = cholesky(Σ).L as LAPACK potrf gives it
 *                     (dpotf2: L21 = Σ21 * (1 / L11)); inv(Σ) of the control cost is getrf + getri
 *                     (MPPIUtils.jl:5-20,45; setup.jl:57)
 * out: U_out[S][H][2]       MPPI.r.Control (= MPPICtrl)
 *      traj_out[S][H+1][7]  MPPI.r.Traj
 *      cost_out[S]          MPPI.r.cost
 *      feasible_out[S]      MPPI.r.Feasibility (1 = :Feasible)
 *      rollout_count_out[S] MPPI.r.RolloutCount (= m + 1, reference off-by-one)
 *      feasible_count_out[S] MPPI.r.FeasibleTrajCount
 * optional (NULL to skip) — MPPI.p.TrajectoryCollection[1:K] (types.jl:3-8):
 *      coll_traj[S][H+1][7][K], coll_ctrl[S][H][K][2], coll_cost[S][K], coll_feas[S][K]
 *      — structure of arrays, rollout index k fastest (Julia (K, 7, H+1, S) and
 *      (2, K, H, S)): holder k's Trajectory is coll_traj[s][:, :, k] transposed, and a
 *      wavefront's per-step stores for 32 consecutive rollouts are full 128-B lines.
 *      (all K rollouts are written; the planner uses the first m = rollout_count-1).
 * Returns MP_ERR_NUMERIC (after writing outputs) if any rollout cost was NaN.
 */
int mp_mppi_plan(mp_ctx* ctx, const mp_mppi_params* p, int32_t S, const double* X0,
                 const double* goal, const double* U_nom, const double* obstacles,
                 const uint8_t* grid, const double* noise, double* U_out, double* traj_out,
                 double* cost_out, int32_t* feasible_out, int32_t* rollout_count_out,
                 int32_t* feasible_count_out, double* coll_traj, double* coll_ctrl,
                 double* coll_cost, uint8_t* coll_feas);

/* Same contract, DEVICE pointers, asynchronous on the context stream.
 * With p->final_stream = 1, U_out, rollout/feasible counts and the TrajectoryCollection
 * are complete in context-stream order as usual, while traj_out, cost_out and
 * feasible_out (the final rollout, MPPIUtils.jl:192-198) are written by the side stream:
 * read them after mp_ctx_join() (stream order) or mp_ctx_synchronize().  The inputs may
 * be overwritten as soon as the context stream has passed the call (the side stream
 * works on a device snapshot).  The NaN check of the final cost is not reported. */
int mp_mppi_plan_dev(mp_ctx* ctx, const mp_mppi_params* p, int32_t S, const double* X0,
                     const double* goal, const double* U_nom, const double* obstacles,
                     const uint8_t* grid, const double* noise, double* U_out, double* traj_out,
                     double* cost_out, int32_t* feasible_out, int32_t* rollout_count_out,
                     int32_t* feasible_count_out, double* coll_traj, double* coll_ctrl,
                     double* coll_cost, uint8_t* coll_feas);

/*
 * mp_rollout — batched TrajectoryRollout with given controls
 * (MPPIUtils.jl:31-57; DynamicWindow/src/DWAUtils.jl:16-42).
 * ctrl[S][K][H][2] with the H stride given in elements (ctrl_stride_h = 2 for a
 * full control list, 0 for DWA's constant controls [S][K][2]); no clamping.
 * U_nom[S][H][2] is used only when p->ctrl_cost != 0.
 * out: traj[S][K][H+1][7] (optional), cost[S][K], feas[S][K],
 *      argmin[S] (optional; 0-based index of the first minimum of cost[s][:] under Julia's
 *      `isless`, what `minimum` over the holders picks (DWAUtils.jl:152, types.jl:9): a NaN cost
 *      is the greatest value, -0.0 < +0.0, the lowest index among equals.  Not Julia's
 *      `argmin(cost)`, which returns the index of a NaN).
 * p->K is ignored; K is the argument.
 */
int mp_rollout(mp_ctx* ctx, const mp_mppi_params* p, int32_t S, int32_t K, const double* X0,
               const double* goal, const double* ctrl, int64_t ctrl_stride_h,
               const double* U_nom, const double* obstacles, const uint8_t* grid,
               double* traj, double* cost, uint8_t* feas, int32_t* argmin);

/*
 * mp_vehicle_euler — the closed-loop plant of MPPI/main.jl:259-261 and
 * DynamicWindow/main.jl:155-156: states .+= VehicleDynamics(states, u)*δt for
 * nsteps steps with control ctrl[n][2] held constant (zero-order hold).
 * states[n][7] updated in place; his[n][nsteps][7] (optional) gets every state.
 */
int mp_vehicle_euler(mp_ctx* ctx, int32_t n, double* states, const double* ctrl, double dt,
                     int32_t nsteps, double* his);

/* Closed-loop driver settings (OptimalControl/MPPI/main.jl:14-19,55-83). */
typedef struct mp_mppi_loop_params {
  int32_t update_steps; /* plant steps per replan: update_idx = Int32(floor(update_time/δt)) (main.jl:19) */
  int32_t max_steps;    /* plant steps of the run: Int32(floor(15/δt)) (main.jl:55)                     */
  double plant_dt;      /* δt (main.jl:18)                                                           */
  double goal_radius;   /* stop after the plant step that ends within this distance of goal (main.jl:80: 6) */
  int32_t poll_every;   /* replans enqueued between host checks of the live-scene flags (0: 8)        */
  int32_t reserved;
} mp_mppi_loop_params;

/*
 * mp_mppi_closed_loop — the MPPI closed loop of OptimalControl/MPPI/main.jl:55-83 for S independent
 * scenes (egos) in lockstep, entirely on the device.  Every update_steps plant steps (and at
 * step 1): ShiftInitialCondition(mppi, states); defineMPPINominalControl!(mppi, NominalControls);
 * MPPIPlan(mppi); NominalControls = mppi.r.Control.  Each plant step applies
 * controls[i] = NominalControls[hold_idx[i] + 1, :] (0-based row hold_idx[i] of U; the caller's
 * interpolate(time_serial, ·, Gridded(Constant{Previous}()))(fined_time_serial), main.jl:64-66),
 * i = (time_idx − 1) mod update_steps, and states .+= VehicleDynamics(states, u)·δt (main.jl:74-75).
 * A scene stops after the step whose (x, y) is within goal_radius of its goal (main.jl:77-79);
 * the others go on.  Replan r of every scene uses Philox counter word p->offset + r (MP_NOISE_PHILOX)
 * or the caller's z (MP_NOISE_EXTERNAL).  The final rollout of each plan runs on the side stream
 * (p->final_stream is ignored), beside the plant.
 *
 * in : X0[S][7], goal[S][2], U_nom0[S][H][2] (NominalControls before the first plan),
 *      obstacles[S][n_obs][3], grid[S][ny][nx] as mp_mppi_plan,
 *      hold_idx[update_steps] (0-based rows of U, each in [0, H)),
 *      noise[R][S][K][H][2] (MP_NOISE_EXTERNAL; R = ceil(max_steps / update_steps)) or NULL.
 * out: his[S][max_steps+1][8]  states_his' rows [time_idx·δt, states...]; row 0 = [0, X0]
 *      n_rows[S]               rows written (time steps run + 1)
 *      n_replans[S]            MPPIPlan calls made for the scene
 * optional (NULL to skip), per replan r < n_replans[s]:
 *      U_log[S][R][H][2] (mppi.r.Control), traj_log[S][R][H+1][7] (mppi.r.Traj),
 *      cost_log[S][R] (mppi.r.cost), feas_log[S][R] (mppi.r.Feasibility),
 *      rc_log[S][R] (mppi.r.RolloutCount).
 * Returns MP_ERR_NUMERIC (after writing outputs) if any rollout cost was NaN.
 */
int mp_mppi_closed_loop(mp_ctx* ctx, const mp_mppi_params* p, const mp_mppi_loop_params* lp, int32_t S,
                        const double* X0, const double* goal, const double* U_nom0, const double* obstacles,
                        const uint8_t* grid, const int32_t* hold_idx, const double* noise, double* his,
                        int32_t* n_rows, int32_t* n_replans, double* U_log, double* traj_log, double* cost_log,
                        int32_t* feas_log, int32_t* rc_log);

/* ----------------------------------------------------------- multi-GPU */
/*
 * One host process driving several GPUs (the Julia host of OptimalControl/MPPI/main.jl:59-61 keeps
 * its single process): one context per GPU, joined into one RCCL communicator
 * (ncclCommInitAll over the contexts' devices, xGMI between MI355X GPUs).  ctxs[i] is rank i; every
 * call below takes the same array in the same order.  Errors are reported on ctxs[0]
 * (mp_last_error(ctxs[0])).  RCCL is loaded on first use: MP_ERR_UNSUPPORTED without librccl.
 * Call mp_comm_destroy before destroying the contexts: mp_ctx_destroy refuses (MP_ERR_INVALID) a
 * context that still belongs to a communicator.
 */
int mp_comm_init(mp_ctx** ctxs, int32_t n);
int mp_comm_destroy(mp_ctx** ctxs, int32_t n);
/* ncclAllGather of `bytes` bytes per rank: DEVICE buffers send[i] (on ctxs[i]'s GPU) -> recv[i]
 * ([n][bytes], rank-major), enqueued on every context stream (asynchronous). */
int mp_comm_allgather_dev(mp_ctx** ctxs, int32_t n, void* const* send, void* const* recv, size_t bytes);

/*
 * mp_mppi_plan_sharded — multi-ego MPPIPlan (MPPIUtils.jl:169-203) of S independent scenes sharded over
 * the n GPUs of a communicator: ctxs[r] plans the balanced block [a_r, b_r) of scenes (the first
 * S mod n ranks take one extra) with Philox counter word p->scene_base + a_r — so every scene draws
 * the noise it draws in one mp_mppi_plan over all S — then one RCCL all-gather of the per-scene
 * results (MPPICtrl, final trajectory, cost, flags, counts: (2H + 7(H+1) + 4) doubles per scene) leaves
 * every GPU holding all S scenes' optimal controls; the host outputs are copied from ctxs[0]'s copy.
 * Inputs and outputs as mp_mppi_plan over all S scenes (HOST pointers, synchronous); the
 * TrajectoryCollection stays per GPU and is not returned here.
 */
int mp_mppi_plan_sharded(mp_ctx** ctxs, int32_t n, const mp_mppi_params* p, int32_t S, const double* X0,
                         const double* goal, const double* U_nom, const double* obstacles, const uint8_t* grid,
                         const double* noise, double* U_out, double* traj_out, double* cost_out,
                         int32_t* feasible_out, int32_t* rollout_count_out, int32_t* feasible_count_out);

/* ---------------------------------------------------------------- iLQR */
#define MP_ILQR_NX 4 /* [x, y, ux, ψ]  OptimalControl/ILQR/Dynamics.jl:4-7 */
#define MP_ILQR_NU 2 /* [ax, δ]                                          */
#define MP_ILQR_OPTIMALCONTROL 0 /* OptimalControl/ILQR/Cost.jl           */
#define MP_ILQR_PARKING 1        /* PathPlanning/Parking_ILQR/Cost.jl     */

typedef struct mp_ilqr_params {
  int32_t N;           /* knots per trajectory (ILQR.jl:15: 20; Parking: 30) */
  int32_t variant;     /* MP_ILQR_*: cost weights                            */
  double dT;           /* δT = 0.05                                          */
  double eps;          /* finite-difference step ϵ = 1e-3 (GetMatrix.jl:4)   */
  double alpha_floor;  /* 0: none (ILQR.jl:71-82); 1e-3 Parking_ILQR.jl:83-85 */
  double tol;          /* |ΔJ/J| stop (ILQR.jl:44): 1e-6                     */
  int32_t max_iter;    /* safety cap on outer iterations (reference: none)   */
  int32_t max_ls;      /* safety cap on line-search halvings (reference: none) */
} mp_ilqr_params;

/* Layouts (Julia column-major in parentheses):
 *   X[B][N][4]  (StatesList 4×N per instance)   U[B][N][2]  (CtrlsList 2×N)
 *   k[B][N-1][2]  (klist 2×1×(N-1))              Kg[B][N-1][4][2]  (Klist 2×4×(N-1))  */

/* Initial-guess roll out (ILQR.jl:31-37) + TotalCost (Cost.jl:1-8). */
int mp_ilqr_rollout(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, const double* x0,
                    const double* U, double* X, double* J);
/* One backward Riccati sweep (ILQR.jl:46-67). */
int mp_ilqr_backward(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, const double* X,
                     const double* U, double* k, double* Kg);
/* One forward trial at step size alpha[B] (ILQR.jl:72-80): closed-loop RK4 roll out. */
int mp_ilqr_forward(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, const double* X,
                    const double* U, const double* k, const double* Kg, const double* alpha,
                    double* Xnew, double* Unew, double* Jnew);
/* Same contracts, DEVICE pointers, asynchronous on the context stream. */
int mp_ilqr_backward_dev(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, const double* X,
                         const double* U, double* k, double* Kg);
int mp_ilqr_forward_dev(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, const double* X,
                        const double* U, const double* k, const double* Kg, const double* alpha,
                        double* Xnew, double* Unew, double* Jnew);
/* The whole script loop (ILQR.jl:39-88) per instance: backward + halving line
 * search until |ΔJ/J| <= tol.  X/U in: initial guess; out: solution. */
int mp_ilqr_solve(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, double* X, double* U,
                  double* J, int32_t* iters);
/* Same, DEVICE pointers: X (B,N,4) / U (B,N,2) solved in place, J (B) and iters (B) written on the
 * device.  Synchronous like mp_ilqr_solve (its host loop polls the active count every iteration); it
 * only skips the host transfers -- the form the bench times, inputs resident in HBM. */
int mp_ilqr_solve_dev(mp_ctx* ctx, const mp_ilqr_params* p, int32_t B, double* X, double* U,
                      double* J, int32_t* iters);

/* ---------------------------------------------------------- Hybrid A* */
/* Settings mirror HybridAstarSettings (PathPlanning/HybridAstar/src/types.jl:20-43). */
typedef struct mp_ha_params {
  double vehicle_len, vehicle_wid; /* vehicle_size                               */
  double minR;                     /* minimum turning radius                     */
  double expand_time;              /* primitive length in time (2.5)             */
  double res[3];                   /* resolutions [x, y, ψ]                      */
  double stbound[6];               /* regulated [xmin, xmax, ymin, ymax, ψmin, ψmax] */
  int32_t n_walls;                 /* obstacle blocks per scene, [x,y,ψ,l/2,w/2] */
  int32_t n_prim;                  /* num_neighbors = num_gear*num_steer (62)    */
  int32_t n_col;                   /* primitive path columns (250)               */
  int32_t max_pops;                /* safety cap on search iterations            */
} mp_ha_params;

/* neighbor_origin (hybrid_astar_utils.jl:483-503) computed by the library (FDLIBM sin/cos,
 * Euler Δt = 1e-2, n_col = floor(expand_time/Δt)), returned and installed in the context:
 * states_candi[n_gear*n_steer][3], paths_candi[n_gear*n_steer][n_col][3] (either may be NULL: not
 * returned).  A repeat call with the same settings as the installed table returns its copies without
 * recomputing or re-uploading it (mp_ha_set_primitives clears that memo). */
int mp_ha_neighbor_origin(mp_ctx* ctx, const mp_ha_params* p, int32_t n_steer, const double* steer_set,
                          int32_t n_gear, const double* gear_set, double* states_candi, double* paths_candi);

/* Primitive table of neighbor_origin (hybrid_astar_utils.jl:483-503):
 * states_candi[n_prim][3], paths_candi[n_prim][n_col][3]  (Julia 3×n_prim, 3×n_col×n_prim). */
int mp_ha_set_primitives(mp_ctx* ctx, const mp_ha_params* p, const double* states_candi,
                         const double* paths_candi);

/* Batched FindNewNode device part (hybrid_astar_utils.jl:391-421) for B popped nodes:
 *   node[B][3], goal[B][3] (ending_states), walls[B][n_walls][5]
 * out: nb_states[B][n_prim][3] regulated neighbor states,
 *      idx[B][n_prim]  Encode (0 = out of bounds),
 *      free_[B][n_prim] 1 if in bounds and dg_cost finite (collision free),
 *      h[B][n_prim]     rs_heuristic (valid where free_ == 1).  It stays the Reeds-Shepp heuristic
 *                       alone: astar_heuristic (use_astar) is applied by mp_ha_plan_astar where it
 *                       forms temp_h, from mp_ha_astar_table's table. */
int mp_ha_expand(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* node,
                 const double* goal, const double* walls, double* nb_states, int64_t* idx,
                 uint8_t* free_, double* h);

/* Batched RS_connected (hybrid_astar_utils.jl:224-233): optimal Reeds–Shepp
 * path from node to goal, its 100-steps-per-segment Euler path and the
 * collision check.  path[B][501][3] (first path_len[B] columns valid). */
int mp_ha_rs_connect(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* node,
                     const double* goal, const double* walls, uint8_t* ok, double* path,
                     int32_t* path_len);

/* Whether the collision sweeps of mp_ha_expand / mp_ha_rs_connect / mp_ha_plan use their SAT culls
 * (certain-result SeparatingAxisTheorem calls skipped, CollisionDetection/src/utils.jl:37-74) for these
 * inputs: *active = 1 when every coordinate and length (walls[B][n_walls][5] centres + half extents,
 * stbound, a[B][3] and b[B][3] x/y -- start or node, goal -- minR, vehicle and primitive sizes) is
 * <= 1e6 m, the range the culls' rounding margin is proven for; 0 otherwise (every SAT call runs).
 * Either way the booleans are the reference's.  No device work. */
int mp_ha_sat_cull_active(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* walls, const double* a,
                          const double* b, int32_t* active);

/* allpath (ReedsSheppsCurves/src/ReedsSheppsUtils.jl:468-511) for B normalised
 * states; out: cost[B][48] (Inf where infeasible), cmds[B][48][5][3], best[B]. */
int mp_ha_allpath(mp_ctx* ctx, int32_t B, const double* norm_states, double* cost,
                  double* cmds, int32_t* best);

/* Whole planHybridAstar! search loop (hybrid_astar_utils.jl:235-296) for B
 * scenes in lockstep, entirely on the device: per iteration one fused
 * RS-connect + expansion launch and one bookkeeping launch (Dict, open list in
 * the reference's stable-sort order, popfirst!), enqueued without host round
 * trips.  n_prim <= 64.  start[B][3], goal[B][3] already regulated
 * (setup.jl:110-112).
 * out: found[B], pops[B] (loop_count), n_nodes[B] (length(nodes_collection)),
 *      pop_seq[B][max_pops] (Encode index of each popped node, -1 padded),
 *      n_states[B] and states_out[B][max_pops][3] (hybrid_astar_states, goal→start order),
 *      rs_len[B] and rs_path[B][501][3] (RSpath_final). */
int mp_ha_plan(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* start,
               const double* goal, const double* walls, int32_t* found, int32_t* pops,
               int32_t* n_nodes, int64_t* pop_seq, int32_t* n_states, double* states_out,
               int32_t* rs_len, double* rs_path);

/* astar_heuristic (hybrid_astar_utils.jl:375-387) for B Hybrid A* scenes: the final_cost of planAstar!
 * on the 11 x 11 grid over stbound's x/y box with the scene's walls as block obstacles, from every cell
 * to the cell of goal[B][3]'s (x, y).  planAstar! depends on the state only through its start cell
 * (Astar/src/setup.jl:17), so the heuristic of a state (x, y) of scene b is
 *   table[b][(iy - 1) * 11 + (ix - 1)],  ix = Int(floor((x - xmin) / x_factor + 1)),
 *                                         iy = Int(floor((y - ymin) / y_factor + 1))   (1-based cells),
 * x_factor = (xmax - xmin) / 10.  0.0 where the goal cannot be reached (final_cost's initial value) and
 * in the goal's own cell (see mp_astar_plan).  walls[B][n_walls][5]; n_walls = 0: all cells free. */
int mp_ha_astar_table(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* goal, const double* walls,
                      double* table);

/* mp_ha_plan with HybridAstarSettings.use_astar (types.jl:37).  use_astar = 0: mp_ha_plan exactly.
 * use_astar = 1: the table of mp_ha_astar_table is built on the device ahead of the search and every
 * child's temp_h is max(rs_heuristic, astar_heuristic) (hybrid_astar_utils.jl:419, Julia's max: NaN
 * propagates).  Same outputs as mp_ha_plan. */
int mp_ha_plan_astar(mp_ctx* ctx, const mp_ha_params* p, int32_t B, const double* start,
                     const double* goal, const double* walls, int32_t use_astar, int32_t* found,
                     int32_t* pops, int32_t* n_nodes, int64_t* pop_seq, int32_t* n_states,
                     double* states_out, int32_t* rs_len, double* rs_path);

/* retrievePath + cubic_fit (PathPlanning/HybridAstar/src/hybrid_astar_utils.jl:100-177) for B planned
 * scenarios, one block each: actualpath = [starting_states, cubic_fit(states[:,i], states[:,i+1]) (100
 * points each, i over the hybrid_astar_states reversed to start -> goal order), RSpath_final], its
 * cumulative arc length path_length, tol_length = path_length[end], and the 50 samples of
 * x/y/ψ_interp_dense at LinRange(0, tol_length, 50) that x/y/ψ_interp are built on.
 * in : start[B][3] (starting_states), n_states[B] and states[B][state_stride][3] as mp_ha_plan returns
 *      them (goal side first; n_states = 0: nothing found, nothing retrieved), rs_len[B],
 *      rs_path[B][501][3] (RSpath_final).
 * out: n_points[B] = 1 + 100 (n_states - 1) + rs_len (0 if n_states = 0), tol_length[B],
 *      samples[B][50][3] (x, y, ψ at the 50 arc-length knots).
 * optional (all NULL or path_offset given): path_offset[B+1] (written: scenario b's points are
 *      [path_offset[b], path_offset[b+1])), actualpath[path_offset[B]][3], path_length[path_offset[B]]. */
int mp_ha_retrieve_path(mp_ctx* ctx, int32_t B, const double* start, const int32_t* n_states, const double* states,
                        int32_t state_stride, const int32_t* rs_len, const double* rs_path, int64_t* path_offset,
                        double* actualpath, double* path_length, int32_t* n_points, double* tol_length,
                        double* samples);

/* ------------------------------------------------------------ grid A* */
/* planAstar! (PathPlanning/Astar/src/astar_utils.jl:83-141 with FindNewNode :190-235) for B independent
 * searches on nx x ny grids (defineAstar, Astar/src/setup.jl:3-24), one wavefront per search with its
 * node table and open list in LDS; the free-cell mask (checkObsSafety) of each search's scene is
 * computed once, ahead of it.  nx, ny >= 2 and nx*ny <= 51*51 (MP_ERR_INVALID beyond).
 * in : bound[B][4] (actualbound: xmin, xmax, ymin, ymax), start_real[B][2], goal_real[B][2],
 *      obs_kind 3 (circles [x, y, r]) or 5 (blocks [x, y, psi, l/2, w/2]),
 *      obstacles[B][n_obs][obs_kind].
 * out: final_cost[B], found[B], pops[B] (loop_count), n_nodes[B] (length(nodes_collection)).
 * optional (NULL: not returned):
 *      pop_seq[B][2*(nx*ny+1)]  Encode index, (y-1)*nx + x, of every popped cell, -1 padded
 *                               (0: a start cell off the grid);
 *      astarpath[B][nx*ny+1] with path_n[B] (both or neither): the path's Encode indices, start -> goal;
 *      path_length[B]           astar.r.path_length.
 * Cells, costs and the pop order are the reference's (a stable sort of the open list by f every
 * iteration, nodes updated in place, closed nodes re-opened).  Two inputs on which the reference itself
 * fails are defined here:
 *   - start cell == goal cell: the reference sets final_cost = 0 and then throws KeyError(nothing)
 *     (astar_utils.jl:110); here cost 0, found, a one-cell path of length 0;
 *   - an empty obstacle list (n_obs = 0): the reference indexes obstacle_list[1]; here every cell is free.
 * An unreachable goal (or one off the grid) leaves final_cost = 0.0, found = 0.  The loop is bounded by
 * 2*(nx*ny+1) pops; a search that reaches the bound makes the call return MP_ERR_NUMERIC (outputs
 * written). */
int mp_astar_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                  const double* goal_real, int32_t obs_kind, int32_t n_obs, const double* obstacles,
                  double* final_cost, int32_t* found, int32_t* pops, int32_t* n_nodes, int32_t* pop_seq,
                  int32_t* astarpath, int32_t* path_n, double* path_length);

/* ------------------------------------------------- grid Dijkstra and BFS */
/* planDKA! (PathPlanning/Dijkstra/src/dka_utils.jl:69-126 with FindNewNode :175-215) for B independent
 * searches on nx x ny grids (defineDKA, Dijkstra/src/setup.jl:3-25): planAstar! without the heuristic.  The
 * nine-entry direction list, the stable sort of the open list every iteration, the in-place update and the
 * InOpen rule are mp_astar_plan's; the update test is on f (:193), which with no heuristic is the cost from
 * the start.  One wavefront per search, grid limits and pop bound (MP_ERR_NUMERIC) as for mp_astar_plan.
 * in : bound[B][4], start_real[B][2], goal_real[B][2] as for mp_astar_plan;
 *      circles[B][n_obs][3] ([x, y, r]: checkObsSafety :233-243, strict <); NULL iff n_obs == 0 -- the
 *      reference's loop runs over 1:0 then, every cell is free.
 * out: final_cost[B] (the popped goal node's f), found[B], pops[B] (loop_count), n_nodes[B].
 * optional (NULL: not returned):
 *      pop_seq[B][2*(nx*ny+1)]  Encode index of every popped cell, -1 padded (0: a start cell off the grid);
 *      path[B][nx*ny+1] with path_n[B] (both or neither): dkapath as Encode indices, start -> goal;
 *      path_length[B]           dka.r.path_length (:112), a left fold over actualpath.
 * Defined here where the reference fails or is silent:
 *   - start cell == goal cell (the reference indexes nodes_collection[nothing], :93): found, one pop, a
 *     one-cell path, length 0, cost 0;
 *   - a start one cell off the grid is kept (Encode 0) and can step onto the grid; two cells off: one pop,
 *     not found;
 *   - a goal off the grid is never reached: the search exhausts the reachable cells, found = 0,
 *     final_cost = 0.0. */
int mp_dka_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                const double* goal_real, int32_t n_obs, const double* circles, double* final_cost, int32_t* found,
                int32_t* pops, int32_t* n_nodes, int32_t* pop_seq, int32_t* path, int32_t* path_n,
                double* path_length);

/* planBFS! (PathPlanning/BreadthFirst/src/bfs_utils.jl:1-59 with FindNewNode :137-161) for B independent
 * searches: the four axis moves (:140), a FIFO that is never sorted, a cell enters nodes_collection and the
 * queue once.  One wavefront per search expands a whole level of the queue at a time and keeps the
 * sequential loop's order: the pop sequence, the parents and the node count are the reference's, the nodes
 * queued behind the goal in its level are not expanded.  Arguments, limits and the cases defined above as
 * for mp_dka_plan, without final_cost (BFSNode carries no cost); pops never exceed nx*ny + 1.
 *      path[B][nx*ny+1]   bfspath as Encode indices, start -> goal;
 *      path_length[B]     an extension: BFSResult (BreadthFirst/src/types.jl:32-36) has no path_length; it
 *                         is computed as planDKA! computes it, the same left fold over actualpath. */
int mp_bfs_plan(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, const double* start_real,
                const double* goal_real, int32_t n_obs, const double* circles, int32_t* found, int32_t* pops,
                int32_t* n_nodes, int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length);

/* ------------------------------------- grid planners: large grids, masks */
#define MP_GRID_ASTAR 0
#define MP_GRID_DKA 1
#define MP_GRID_BFS 2
#define MP_GRID_OBS_MASK 1     /* obs_kind: caller-supplied free-cell mask */
#define MP_GRID_FORCE_GLOBAL 1 /* flags bit 0: run the global-memory kernels whatever the size */
#define MP_GRID_MAX_CELLS (1 << 22)

/* mp_astar_plan / mp_dka_plan / mp_bfs_plan (planner = MP_GRID_ASTAR / MP_GRID_DKA / MP_GRID_BFS) without the
 * 51 x 51 limit, and with occupancy masks.  Arguments, output layouts, optional outputs, the pop bound
 * 2*(nx*ny+1) (MP_ERR_NUMERIC) and the cases defined where the reference fails are those of the three calls
 * above; final_cost may be NULL for MP_GRID_BFS and is ignored there.
 *   nx, ny >= 2 and nx*ny <= MP_GRID_MAX_CELLS (MP_ERR_INVALID beyond).
 *   obs_kind 3 (circles): every planner.  obs_kind 5 (blocks): MP_GRID_ASTAR only, as in the reference
 *     (MP_ERR_INVALID with the other two).
 *   obs_kind MP_GRID_OBS_MASK: obstacles is const uint8_t mask[B][ny][nx], cell (ix, iy) at (iy-1)*nx + ix-1,
 *     nonzero = free; n_obs is ignored.  An extension: the result is the reference planner's with
 *     checkObsSafety replaced by the table lookup.
 * With nx*ny <= 51*51 and MP_GRID_FORCE_GLOBAL clear the searches run the kernels of the three calls above (one
 * wavefront each, node table in LDS).  Otherwise one workgroup runs each search on node tables in a device
 * workspace: 32 bytes per cell and search for A* and Dijkstra, 12 for BFS, beside the outputs' 12.  A* and
 * Dijkstra pop the open entry with the smallest (f, number), numbers handed out so that the order is the
 * reference's stable sort; every output is the same either way.  A workspace that cannot
 * be had (mp_ctx_set_workspace_limit, or the device is full) returns MP_ERR_NOMEM before anything is launched. */
int mp_grid_plan(mp_ctx* ctx, int32_t planner, int32_t flags, int32_t B, int32_t nx, int32_t ny, const double* bound,
                 const double* start_real, const double* goal_real, int32_t obs_kind, int32_t n_obs,
                 const void* obstacles, double* final_cost, int32_t* found, int32_t* pops, int32_t* n_nodes,
                 int32_t* pop_seq, int32_t* path, int32_t* path_n, double* path_length);

/* ------------------------------------------------------- occupancy maps */
#define MP_MAP_BORDER 1                   /* flags bit 0: a one-cell frame around the map counts as blocked */
#define MP_MAP_OUT_OCCUPIED 2             /* flags bit 1 (mp_grid_inflate): write 1 = occupied, MPPI's polarity */
#define MP_MAP_D2_NONE 2147483647         /* d2 of a map with no blocked cell (INT32_MAX) */
#define MP_MAP_MAX_BATCH_CELLS (1 << 28)  /* B*nx*ny of one call */
#define MP_MAP_MAX_SIDE 32768             /* nx, ny of the three distance calls: d2 fits int32, a row distance uint16 */

/* Tools on the maps the grid planners and MPPI take (an extension: the reference has none of them).
 *
 * A map is uint8_t mask[ny][nx], the planners' convention: cell (ix, iy) (1-based) at (iy-1)*nx + ix-1, any
 * nonzero byte = free.  d2[ny][nx] (int32) is the squared Euclidean distance, in cells, from each cell to the
 * nearest blocked cell: 0 on a blocked cell, MP_MAP_D2_NONE everywhere on a map without one.  Cells count as
 * square and distances are in cells, not metres.  With MP_MAP_BORDER the cells of a one-cell frame around the
 * map (ix = 0, nx+1, iy = 0, ny+1) are blocked too: d2 <= min(ix, nx+1-ix, iy, ny+1-iy)^2 and no cell has
 * MP_MAP_D2_NONE.  Everything is integer-exact: the outputs do not depend on the batch, the device or the
 * algorithm.
 *
 * All four calls take host pointers and run on the context's stream (they return after the copy back).
 *   B >= 1, nx, ny >= 2, nx*ny <= MP_GRID_MAX_CELLS, B*nx*ny <= MP_MAP_MAX_BATCH_CELLS; for the three distance
 *   calls also nx, ny <= MP_MAP_MAX_SIDE (beyond it a distance along a row does not fit 16 bits, nor d2 32).
 *   A limit exceeded, an unknown flag bit, a NULL pointer or a negative r2: MP_ERR_INVALID, nothing launched or
 *   written.  A workspace that cannot be had (mp_ctx_set_workspace_limit, or the device is full): MP_ERR_NOMEM,
 *   nothing launched or written.  Workspaces per cell of the batch: mp_grid_distance 7 bytes, mp_grid_inflate
 *   4, mp_grid_path_clearance 7 beside the paths.
 *
 * mp_grid_rasterize: the masks mp_astar_plan / mp_dka_plan / mp_bfs_plan / mp_grid_plan build for themselves from
 *   bound[B][4] and obstacles[B][n_obs][obs_kind] (3: circles [x, y, r]; 5: blocks [x, y, psi, l/2, w/2], A*'s
 *   checkObsSafety), byte for byte (0 / 1).  n_obs = 0 (obstacles may be NULL): every cell free.
 * mp_grid_distance: d2[B][ny][nx] of mask[B][ny][nx].  flags: MP_MAP_BORDER.
 * mp_grid_inflate: mask_out[B][ny][nx], 1 = free iff the cell is free in mask and d2 > r2[b] (r2 >= 0, one per
 *   map; r2 = 0 returns mask normalised to 0 / 1; a disc of radius r cells is r2 = floor(r^2)).  With
 *   MP_MAP_OUT_OCCUPIED the bytes are inverted, 1 = occupied (mp_mppi_plan's grid).  d2 is never written out: the
 *   search for the nearest blocked cell stops where the verdict is known.  flags: MP_MAP_BORDER,
 *   MP_MAP_OUT_OCCUPIED.
 * mp_grid_path_clearance: path[B][stride] holds paths as mp_grid_plan writes them (stride >= 1), Encode values
 *   1..nx*ny; only the first path_n[b] (0 .. stride) entries are read, an entry of 0 (a start off the map) is
 *   skipped, any other entry outside 1..nx*ny is MP_ERR_INVALID.  min_d2[b] is the least d2 of map b over the
 *   path's cells, at[b] the (0-based) index of the first entry that attains it; an empty path, or one skipped
 *   entirely: MP_MAP_D2_NONE and -1.  flags: MP_MAP_BORDER. */
int mp_grid_rasterize(mp_ctx* ctx, int32_t B, int32_t nx, int32_t ny, const double* bound, int32_t obs_kind,
                      int32_t n_obs, const double* obstacles, uint8_t* mask);
int mp_grid_distance(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask, int32_t* d2);
int mp_grid_inflate(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask,
                    const int32_t* r2, uint8_t* mask_out);
int mp_grid_path_clearance(mp_ctx* ctx, int32_t flags, int32_t B, int32_t nx, int32_t ny, const uint8_t* mask,
                           const int32_t* path, const int32_t* path_n, int32_t stride, int32_t* min_d2, int32_t* at);

/* ------------------------------------------------- goal-distance fields */
#define MP_FIELD_TO_SOURCE 1                /* flags bit 0: the cost of travelling from each cell to the source */
#define MP_FIELD_MOVES_REF 0x7F             /* dka_utils.jl:177's seven distinct moves (no (-1, +1)) */
#define MP_FIELD_MOVES_8 0xFF
#define MP_FIELD_MOVES_4 0x69
#define MP_FIELD_MAX_BATCH_CELLS (1 << 26)  /* B*nx*ny of one call: 512 MiB of field */

/* The cost from one source cell to every cell of each of B occupancy maps, and paths read off it (an extension:
 * planDKA! run until its open list is empty leaves these labels in nodes_collection, dka_utils.jl:73).
 *
 * Geometry (bound[B][4], nx, ny, factors, real -> cell) is mp_grid_plan's, mask[B][ny][nx] that of
 * MP_GRID_OBS_MASK.  moves is a set over the neighbours (dx, dy), bit 0 .. bit 7:
 *   (-1,0) (-1,-1) (1,-1) (1,0) (1,1) (0,-1) (0,1) (-1,1)
 * and move d costs c(d) = sqrt(double(dx^2)*(xf*xf) + double(dy^2)*(yf*yf)) (dka_utils.jl:189).  A cell is a member
 * iff it is on the grid and its mask byte is nonzero, or it is the source (the reference never tests its start).
 * field[source] = 0; every other member holds the unique solution of f[v] = min over moves u -> v of
 * fl(f[u] + c(u -> v)) in IEEE double -- bit for bit planDKA!'s final_cost to v with MP_FIELD_MOVES_REF --;
 * non-members and unreached members hold +Inf.  n_reached[b] counts the finite cells.  A source off the grid gives
 * an all-+Inf field and n_reached = 0 (mp_dka_plan keeps a start one cell outside; this call does not).
 * With MP_FIELD_TO_SOURCE the graph is reversed: f[v] = min over d of fl(f[v + d] + c(d)), the cost of travelling
 * from v to the source; the sum accumulates from the source, so it is not claimed equal to planDKA! from v.
 *
 * Queries: query q reads map q_map[q] at the cell of q_real[q].  q_cost[q] is the field there; +Inf and
 * path_n = 0 when the cell is off the grid or unreached.  The path is in travel order, as Encode indices (it feeds
 * mp_grid_path_clearance unchanged): source -> query, built backwards by taking from v the lowest-bit move d with
 * u = v - d finite and fl(f[u] + c(d)) == f[v]; with MP_FIELD_TO_SOURCE query -> source, u = v + d.  path_n[q] is
 * the full length; only the first min(path_n, stride) entries of path[q][stride] are written.  path_length[q] is
 * the planners' left fold over the TransferCoordinate rows of the whole path.
 *
 *   flags: MP_FIELD_TO_SOURCE.  moves: 1 .. 0xFF.  B >= 1, nx, ny >= 2, nx*ny <= MP_GRID_MAX_CELLS,
 *   B*nx*ny <= MP_FIELD_MAX_BATCH_CELLS; finite bounds and positive factors; Q >= 0, q_map in 0 .. B-1.
 *   field and n_reached may each be NULL; Q = 0 takes every query pointer NULL; Q > 0 needs q_map, q_real and
 *   q_cost; path, path_n and path_length come all together (stride >= 1) or not at all.  At least one output must
 *   be asked for.  A violation: MP_ERR_INVALID, nothing launched or written.  A workspace that cannot be had:
 *   MP_ERR_NOMEM, nothing launched or written.  Workspaces: 9 bytes per cell of the batch; with paths also
 *   4 bytes per query and member cell of its map.  More than nx*ny + 1 relaxation rounds: MP_ERR_NUMERIC (it
 *   cannot happen: a round settles at least the cells one more move away). */
int mp_grid_field(mp_ctx* ctx, int32_t flags, int32_t moves, int32_t B, int32_t nx, int32_t ny, const double* bound,
                  const double* source_real, const uint8_t* mask, double* field, int32_t* n_reached, int32_t Q,
                  const int32_t* q_map, const double* q_real, int32_t stride, double* q_cost, int32_t* path,
                  int32_t* path_n, double* path_length);

/* ----------------------------------------------------------- RRT / RRT* */
#define MP_RRT_MAX_ITER 1000000 /* cap on n_iter (the tree workspace is 48 bytes per node and scene; 64 for mp_rrtnh_plan) */

/* Settings mirror RRTSettings (PathPlanning/RRT/src/types.jl:19-39). */
typedef struct mp_rrt_params {
  int32_t n_iter;        /* sampling_number; 1 .. MP_RRT_MAX_ITER               */
  int32_t buffer_size;   /* nodes registered between BallTree rebuilds; >= 1    */
  int32_t rrt_star;      /* 0: RRT, 1: RRT* (near set + rewire)                 */
  int32_t reserved;
  double bias_rate, grow_min, grow_max, goal_tolerance; /* grow_dist = [grow_min, grow_max] */
} mp_rrt_params;
/* Alias of mp_rrt_params, the name mp_rrt_plan's prototype uses; the two are one type. */
typedef mp_rrt_params mp_rrt_params_t;

/*
 * mp_rrt_plan — planRRT! (PathPlanning/RRT/src/rrt_utils.jl:341-412) for B independent scenes in one
 * launch, one workgroup per scene, the whole sampling loop on the device: sampleRRT (:18-39), the nearest
 * node of the BallTree snapshot (rebuilt every buffer_size registered nodes, :386-389 -- between rebuilds
 * the newer nodes are not seen, as in the reference), steer (:159-191) with ProjectionStates (:112-134),
 * collision (:282-311: the bound test on the new point, then both end points against every circle with <=),
 * registerNode, and with rrt_star the near set (:374-377), rewire (:216-238, root_idx = min_idx) and
 * costPropogation (:240-268); then findBestIdx (:414-422) over all nodes and getBestIdxs.
 * in : bound[B][4] (BoundPosition: xmin, xmax, ymin, ymax), start[B][2], goal[B][2],
 *      obstacles[B][n_obs][3] circles [x, y, r]; obs_count[B] (NULL: n_obs each) circles of scene b that
 *      count, the rest of its rows is padding and is not read; n_obs = 0: no obstacles,
 *      uniforms[B][n_iter][3]: (u_bias, u_x, u_y) in [0, 1) per iteration.  The library draws no random
 *      numbers: u_bias < bias_rate makes the sample the goal (u_x, u_y ignored, where the reference does
 *      not draw them), otherwise it is (u_x*(xmax-xmin)+xmin, u_y*(ymax-ymin)+ymin).
 * out: n_nodes[B] (sample_idx), status[B] (1 :Solved, 0 :NotSolved), best_idx[B] (0 when not solved),
 *      best_cost[B] (costs_collection[best_idx]; 0.0 when not solved).
 * optional (NULL: not returned), node i (1-based, as the reference) in row i - 1, rows past n_nodes zero:
 *      loc[B][n_iter+1][2], cost[B][n_iter+1], parent[B][n_iter+1] (node 1: -1),
 *      path_idx[B][n_iter+1] with path_n[B] (both or neither): getBestIdxs, goal side first, ending in 1,
 *      counters[B][4]: samples rejected by collision, rewired edges, near sets that reached the cap of
 *      100, steers that took the in-range branch.
 * Defined differently from the reference:
 *   - tree queries: NearestNeighbors' knn / inrange (their tie order and the last-ulp pruning of their
 *     trees) are brute force over the same nodes: the nearest node is the minimum of dx*dx + dy*dy, the
 *     lowest index on ties; the near set is every snapshot node with sqrt(dx*dx + dy*dy) <= r, and from
 *     100 such nodes on the 100 nearest by (distance, index); the goal set is dx*dx + dy*dy <=
 *     goal_tolerance^2, minimum cost, lowest index on ties;
 *   - nearDisk's ^(0.5) is sqrt;
 *   - the 100 s wall-clock break (:391-394) is dropped: all n_iter samples are drawn;
 *   - node capacity: the reference's arrays hold sampling_number nodes and it writes node
 *     sampling_number + 1 out of bounds when every sample registers; here the capacity is n_iter + 1.
 * round(v, digits = 2) is rint(v*100.0)/100.0 and norm of a 2-vector is sqrt(v1*v1 + v2*v2).
 * n_iter outside 1 .. MP_RRT_MAX_ITER, buffer_size < 1 and non-finite bounds, start or goal return
 * MP_ERR_INVALID before anything is launched. */
int mp_rrt_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                double* loc, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n,
                int32_t* counters);

/*
 * mp_rrtnh_plan — planRRT! of the car-like planner (PathPlanning/RRTNonholonomic/src/rrt_utils.jl:528-583) for B
 * independent scenes in one launch, one workgroup per scene, the whole sampling loop on the device.  Nodes are
 * poses [x, y, psi].  Per iteration: sampleRRT (:18-44); the nearest pose of the BallTree snapshot under
 * MyMetrics (types.jl:9-23; the snapshot is rebuilt every buffer_size registered nodes, :558-561); steer
 * (:292-365, both branches, the |dx| <= 0.01 -> 0.01 clamp, adjustdist = grow_max) with ProjectionStates
 * (:208-238), get_max_ang_ratio, get_max_yawangle, DistToDeltaXY, decide_proj and FromProj2Real; collision
 * (:458-498) in the reference's order: the bound test on the second pose, InitialCheck && FeasibilityClassifier
 * on the rounded projection of the directed edge (the classifier's one-sided theta test as written there), then
 * both end points against every circle with <=; registerNode; with rrt_star the near set (:546-549), rewire
 * (:392-414: root_idx = min_idx, the cost of ProjectionStates(near, new), the test collision(new, near);
 * chooseParents stays unused, as there) and costPropogation (:416-431).  Then findBestIdx (:585-593) over all
 * nodes by (x, y) and getBestIdxs.  The settings are mp_rrt_params (RRTSettings has the same live fields; the
 * reference's grow_dist is [1, 3]).
 * Constants, as in the reference: the near-set cap 30 (:547), the radius cap 24 (:372, nearDisk = min(gamma *
 * (log n / n), 24), gamma = 6*W*H*5, n = sample_idx after registering), max_ang = 0.1 (:116), InitialCheck's box
 * dx in [1, 3], dy in [-1, 1], dpsi in [-0.35, 0.35] (:240-258), and get_max_yawangle's two cubics (:120-145).
 * in : bound[B][4] (xmin, xmax, ymin, ymax), start[B][3] (x, y, psi), goal[B][2] (ending_ang is never read by
 *      planRRT!), obstacles / obs_count / n_obs as mp_rrt_plan,
 *      uniforms[B][n_iter][6]: (u_bias, u_x, u_y, u_psi, u_ratio, u_yaw) in [0, 1) per iteration, in the
 *      reference's draw order.  The library draws no random numbers: u_bias < bias_rate makes the sample the
 *      goal, otherwise it is (u_x*(xmax-xmin)+xmin, u_y*(ymax-ymin)+ymin); psi = (u_psi-0.5)*2*pi either way;
 *      u_ratio is used only where steer draws ang_ratio (:309, :350), u_yaw always (:287).  Slots the
 *      reference would not draw are ignored.
 * out: n_nodes[B], status[B] (1 :Solved, 0 :NotSolved), best_idx[B] (0 when not solved), best_cost[B] (0.0
 *      when not solved).
 * optional (NULL: not returned), node i (1-based) in row i - 1, rows past n_nodes zero:
 *      state[B][n_iter+1][3], cost[B][n_iter+1], parent[B][n_iter+1] (node 1: -1),
 *      path_idx[B][n_iter+1] with path_n[B] (both or neither): getBestIdxs, goal side first, ending in 1,
 *      counters[B][8]: 0 samples rejected by the bound test, 1 by kinematics, 2 by a circle, 3 rewired edges,
 *      4 near sets that reached the cap, 5 steers on the in-range branch, 6 steers that drew ang_ratio, 7 near
 *      sets whose radius was below 24.
 * Defined differently from the reference:
 *   - tree queries are brute force over the snapshot under MyMetrics: the nearest node is the minimum metric
 *     value, the lowest index on ties; the near set is every snapshot node with metric <= r, and from 30 such
 *     nodes on the 30 smallest by (metric, index).  MyMetrics is not a metric, so the pruning of
 *     NearestNeighbors' BallTree has no defined answer to pin against: a deviation, not an approximation.  The
 *     goal set is dx*dx + dy*dy <= goal_tolerance^2, minimum cost, lowest index on ties;
 *   - the 100 s wall-clock break (:563-566) is dropped: all n_iter samples are drawn;
 *   - the node capacity is n_iter + 1.
 * round(v, digits = d) is rint(v*10^d)/10^d, x^2 and x^3 are x*x and x*x*x, n-ary + and * fold left, norm of a
 * 2-vector is sqrt(v1*v1 + v2*v2) and dot of two 2-vectors is fma(x1, y1, x0*y0).  neural_cost of a zero
 * distance is Inf or NaN by IEEE, and then no comparison passes.
 * Errors are mp_rrt_plan's: n_iter outside 1 .. MP_RRT_MAX_ITER, buffer_size < 1 and non-finite bounds, start
 * or goal return MP_ERR_INVALID before anything is launched or written; a propagation queue longer than the
 * node count returns MP_ERR_NUMERIC. */
int mp_rrtnh_plan(mp_ctx* ctx, const mp_rrt_params_t* p, int32_t B, const double* bound, const double* start,
                  const double* goal, int32_t n_obs, const int32_t* obs_count, const double* obstacles,
                  const double* uniforms, int32_t* n_nodes, int32_t* status, int32_t* best_idx, double* best_cost,
                  double* state, double* cost, int32_t* parent, int32_t* path_idx, int32_t* path_n,
                  int32_t* counters);

/* ------------------------------------------------------- path tracker */
/* Settings of the Hybrid A* path tracker (PathPlanning/HybridAstar/main_Tracker.jl:42-72). */
typedef struct mp_track_params {
  int32_t n_ref;      /* refined_length = LinRange(0, tol_length, n_ref): 1000 (:42); <= 2048           */
  int32_t max_steps;  /* safety cap on simulation steps (the reference loops until the closest point
                         is the last one, :84)                                                          */
  double dt_sim;      /* 1e-3 (:67)                                                                     */
  double look_ahead;  /* look_ahead_dist 1.0 (:57)                                                      */
  double p_gain;      /* 10 (:58)                                                                       */
  double i_gain;      /* 0.1 (:59)                                                                      */
  double veh_len;     /* veh_param[1] = vehicle_size[1] (:50)                                           */
  double max_sa;      /* veh_param[3] = max_δf + 0.1 (:52)                                              */
  int32_t his_stride; /* states_his: keep the state after every his_stride-th update (0: none)          */
  int32_t reserved;
} mp_track_params;

#define MP_TRACK_DONE 0    /* the closest reference point reached the last one (main_Tracker.jl:84-89) */
#define MP_TRACK_MAXSTEP 1 /* max_steps simulation steps ran without reaching it                         */
#define MP_TRACK_NOPATH 2  /* tol_length not > 0 (no planned path: "Can't find a path", :31-35)         */
#define MP_TRACK_EMPTY 3   /* an empty findclosest window (argmin of an empty range: a Julia error)      */

/*
 * mp_ha_track — the HA* -> tracker hand-off and the tracker closed loop of
 * PathPlanning/HybridAstar/main_Tracker.jl:42-137 for B planned scenarios in lockstep, one wavefront
 * each.  x_ref/y_ref/ψ_ref = x/y/ψ_interp(refined_length) (:42-46, Interpolations.jl linear
 * interpolation on the n_samples knots LinRange(0, tol_length, n_samples)); then per step
 * (simulation_idx = 1, 2, ...): findclosest (tracker_utils.jl:38-43) inside the time windows of
 * :82-90, inverseKinematic (tracker_utils.jl:15-36), the look-ahead point and its findclosest
 * (:97-108), the cross-track PI correction with clamp (:110-119) and the kinematic Euler step
 * (tracker_utils.jl:1-13, :121).
 * in : start_real[B][3] (cur_states = starting_real, :64), tol_length[B] and samples[B][n_samples][3]
 *      as mp_ha_retrieve_path returns them (x/y/ψ_interp values at their knots).
 * out: n_steps[B] (simulation_idx when the loop ended), status[B] (MP_TRACK_*),
 *      final_state[B][3] (cur_states), err_acc[B] (err_accumulated),
 * optional (NULL to skip): ref_out[B][n_ref][3] (x_ref, y_ref, ψ_ref: the hand-off),
 *      his[B][his_cap][3]: states_his (:122) every his_stride-th update, row 0 = starting_real;
 *      rows written = min(his_cap, (n_steps - 1) / his_stride + 1).
 */
int mp_ha_track(mp_ctx* ctx, const mp_track_params* p, int32_t B, const double* start_real,
                const double* tol_length, const double* samples, int32_t n_samples, int32_t* n_steps,
                int32_t* status, double* final_state, double* err_acc, double* ref_out, double* his,
                int32_t his_cap);

/* -------------------------------------------------- collision detection */
/* PathPlanning/CollisionDetection/src/utils.jl (GetRectanglePts, Block2Pts, SeparatingAxisTheorem,
 * ConvexCollision) and Hybrid A*'s block_collision_check (hybrid_astar_utils.jl:180-204) as batched calls.
 * Every product is rounded as the reference's BLAS rounds it: R*pts of GetRectanglePts is dgemm with K = 2,
 * fma(a1, b1, a0*b0); the projections transpose(pts .- bg_pt)*normal_vec are dgemv 'T' on two rows,
 * fma(p_x - bg_x, n_x, (p_y - bg_y)*n_y).  Results are bit for bit the reference's. */
#define MP_COLLIDE_MAX_COLS 32   /* columns (vertices incl. a closing one) per polygon */
#define MP_SAT_BOTH   0          /* ConvexCollision, utils.jl:64-74: SAT(a,b) && SAT(b,a)          */
#define MP_SAT_EITHER 1          /* extension: SAT(a,b) || SAT(b,a), the geometric test            */
#define MP_SAT_BASE_A 2          /* SeparatingAxisTheorem(a, b) alone, utils.jl:37-62              */

typedef struct mp_collide_params {
  double half_len, half_wid;   /* vehicle_size[1]/2, vehicle_size[2]/2                              */
  double center_shift;         /* pose point -> rectangle centre along the heading; reference: half_len */
  int32_t stride;              /* sparcity_num; reference 5; >= 1                                   */
  int32_t mode;                /* MP_SAT_*                                                          */
} mp_collide_params;
/* Alias of mp_collide_params, the name mp_path_collision's prototype uses; the two are one type. */
typedef mp_collide_params mp_collide_params_t;

/* GetRectanglePts (utils.jl:14-25) of n blocks [x, y, ψ, l, w]: pts[n][5][2], Julia's 2x5 matrix per block
 * (UpLeft, LowerLeft, LowerRight, UpperRight, UpLeft again); Block2Pts is the same over a list.  A non-finite
 * block value returns MP_ERR_INVALID; n = 0 returns MP_OK. */
int mp_block_pts(mp_ctx* ctx, int64_t n, const double* blocks, double* pts);

/* ConvexCollision / SeparatingAxisTheorem for every pair (a_i, b_j) of B scenes:
 *   polys_a[B][na][ma][2], polys_b[B][nb][mb][2]: a polygon is its column list as given (a Julia 2 x cols
 *   matrix); a_cols[B][na] / b_cols[B][nb] are the column counts (NULL: ma / mb each), 2 <= cols <=
 *   min(ma or mb, MP_COLLIDE_MAX_COLS); rows past cols are padding and are never read.
 *   SeparatingAxisTheorem(base, other) walks the cols - 1 edges between consecutive columns of base and
 *   projects all columns of both polygons on each edge normal (-v_y, v_x); the caller closes a polygon by
 *   repeating its first point, as the reference does.  An edge separates when
 *   max_other <= min_base || max_base <= min_other; the first separating edge ends the walk.
 * out: free_[B][na][nb] = 1 where the function selected by mode returns true (no collision).
 * As in the reference, two shapes that touch are separated, and a zero-length edge (a repeated vertex) has a
 * zero normal and separates anything.  minimum / maximum are Julia's: a NaN projection (from an overflow)
 * makes neither comparison of its edge hold.
 * MP_ERR_INVALID, with nothing written: a non-finite value in a row that is read, cols out of range, an
 * unknown mode, a negative size.  B = 0 or na*nb = 0 returns MP_OK. */
int mp_convex_collision(mp_ctx* ctx, int32_t mode, int32_t B, int32_t na, int32_t ma, const double* polys_a,
                        const int32_t* a_cols, int32_t nb, int32_t mb, const double* polys_b, const int32_t* b_cols,
                        uint8_t* free_);

/* block_collision_check (hybrid_astar_utils.jl:180-204) for B scenes:
 *   poses[B][n_poses][3] ([x, y, ψ]), pose_count[B] (NULL: n_poses each) poses of scene b that count,
 *   walls[B][n_walls][5] ([x, y, ψ, l/2, w/2]), wall_count[B] (NULL: n_walls each); rows past a count are
 *   padding and are never read.
 * With cnt = pose_count[b]: cnt > stride checks poses 0, stride, 2 stride, ... below cnt; otherwise pose 0
 * alone (the reference's else branch); cnt = 0 checks nothing.  A checked pose becomes the block
 * [x + center_shift cos ψ, y + center_shift sin ψ, modπ(ψ), half_len, half_wid] and is tested against every
 * wall of its scene as (a, b) = (wall, vehicle) under p->mode.  n_walls = 0: every scene is free.
 * out: scene_free[B]  the reference's return value (1 = no checked pose hits a wall),
 *      first_pose[B]  the lowest checked pose index that hits a wall, -1 if none,
 *      first_wall[B]  the lowest wall index that pose hits, -1 if none,
 *      n_hit[B]       checked poses that hit at least one wall,
 *      pose_free[B][n_poses] (optional, NULL to skip): 1 free, 0 hit, 2 not checked.
 * MP_ERR_INVALID, with nothing written: a non-finite value in a checked pose, a counted wall or the
 * settings, a count outside its range, stride < 1, an unknown mode, a negative size.  B = 0 returns MP_OK. */
int mp_path_collision(mp_ctx* ctx, const mp_collide_params_t* p, int32_t B, int32_t n_poses, const double* poses,
                      const int32_t* pose_count, int32_t n_walls, const int32_t* wall_count, const double* walls,
                      uint8_t* scene_free, int32_t* first_pose, int32_t* first_wall, int32_t* n_hit,
                      uint8_t* pose_free);

/* ---------------------------------------------------------- Reeds-Shepp curves */
/* PathPlanning/ReedsSheppsCurves (main.jl, src/ReedsSheppsUtils.jl) for many pose pairs at once.  Poses are
 * [x, y, ψ]; a command table is [5][3] with rows [length, gear, steer] (Julia's 3x5 matrix), candidates are
 * numbered 0..47 as allpath numbers them (4*(word - 1) + variant: plain, timeflip, reflect, reverse).
 * Every value is the reference's in fp64.  Common errors, MP_ERR_INVALID with nothing written: a NULL
 * argument that is not marked optional, a count below 1.  An output above the context's workspace limit:
 * MP_ERR_NOMEM. */

/* ReedsSheppsCurves/main.jl:15-17 for B pose pairs: changeBasis on the device, allpath, argmin.
 * init[B][3], term[B][3], minR[B] (any sign; IEEE results flow through as in mp_ha_allpath).
 * out: norm[B][3] (NULL: not returned), cost[B][48], cmds[B][48][5][3] (NULL: not returned),
 *      best[B] (Julia findmin: first NaN, else first minimum), act_cost[B] = cost[best]*minR. */
int mp_rs_allpath(mp_ctx* ctx, int32_t B, const double* init, const double* term, const double* minR,
                  double* norm, double* cost, double* cmds, int32_t* best, double* act_cost);

/* createPath / createActPath (ReedsSheppsUtils.jl:411-466) for n command tables cmds[n][5][3]
 * (rows up to the first with gear == 0 count, later rows are ignored).
 * init[n][3] and minR[n] both given: createActPath.  Both NULL: createPath (start [0,0,0], no scaling).
 * One NULL only: MP_ERR_INVALID.
 * out: path_len[n] = 100*nseg + 1 (1 for an all-zero table: the start alone),
 *      path[n][501][3]; columns from path_len on are 0.0. */
int mp_rs_create_path(mp_ctx* ctx, int64_t n, const double* init, const double* minR, const double* cmds,
                      double* path, int32_t* path_len);

/* The Reeds-Shepp distance (rs_heuristic, hybrid_astar_utils.jl:361-373: opt_cost*minR) from every
 * a[na][3] to every b[nb][3] at one minR.
 * out: dist[na][nb]; best[na][nb] (candidate index 0..47; NULL: not returned). */
int mp_rs_cost_matrix(mp_ctx* ctx, int32_t na, const double* a, int32_t nb, const double* b, double minR,
                      double* dist, uint8_t* best);

/* ---------------------------------------------------------- Reeds-Shepp roadmap */
/* A multi-query roadmap planner for a car (PRM under the Reeds-Shepp metric): a build extension, the reference
 * has no such planner.  Every edge has the reference's semantics: its length d(a -> b) is mp_rs_cost_matrix's
 * value, and it is free iff RS_connected (hybrid_astar_utils.jl:224-233) holds for the pose pair: createActPath of
 * the winning candidate, block_collision_check at sparcity_num = 5 with the rectangle centre vehicle_len/2 ahead
 * of the pose and ConvexCollision's && of both SATs.  A non-finite d (identical poses give NaN) is no candidate.
 *   nodes[n][3] poses [x, y, ψ], 1 <= n <= MP_ROADMAP_MAX_NODES (a node's n distances are ranked in 32 KB of LDS);
 *   walls[n_walls][5] blocks [x, y, ψ, l/2, w/2], any count (NULL with n_walls = 0); minR finite and > 0;
 *   1 <= k <= MP_ROADMAP_MAX_K.
 * Common errors, MP_ERR_INVALID with nothing written: a NULL argument, a count out of range, a non-finite pose,
 * wall or vehicle size, minR not finite and positive.  An output above the workspace limit: MP_ERR_NOMEM. */
#define MP_ROADMAP_MAX_NODES 4096
#define MP_ROADMAP_MAX_K 64
#define MP_ROADMAP_MAX_QUERIES 65535

/* The directed roadmap: nbr[n][k], row i = the k nodes j != i with the smallest finite d(i -> j), ordered by
 * (d, j) and padded with -1; w[n][k] = d where the edge is free, +Inf where it is blocked or padding. */
int mp_roadmap_build(mp_ctx* ctx, int32_t n, const double* nodes, int32_t n_walls, const double* walls, double minR,
                     double vehicle_len, double vehicle_wid, int32_t k, int32_t* nbr, double* w);

/* B queries start[B][3] -> goal[B][3] on a roadmap (nbr, w) of the same scene, 1 <= B <= MP_ROADMAP_MAX_QUERIES.
 * Vertices: 0 = start, 1..n = nodes, n + 1 = goal.  The start joins the k nodes nearest from it (d(start -> j)),
 * the k nodes with the smallest d(j -> goal) join the goal, both ranked as a build ranks and edge-checked, and the
 * direct edge start -> goal is checked unless its d is not finite.  Dijkstra in fp64: settle the unsettled vertex
 * of smallest finite dist (lowest vertex on ties) until the goal is settled or none is left; an edge relaxes on
 * dist[u] + w < dist[v].  The entries of a row of nbr other than -1 are distinct, as a build returns them.
 * out: found[B], cost[B] (dist[goal], +Inf when not found), seq[B][n + 2] (the vertices from start to goal, -1 from
 *      seq_len on), seq_len[B] (0 when not found), settled[B] (vertices settled), direct_free[B].
 * MP_ERR_INVALID also for an entry of nbr outside -1..n-1 and a non-finite start or goal. */
int mp_roadmap_query(mp_ctx* ctx, int32_t n, const double* nodes, int32_t n_walls, const double* walls, double minR,
                     double vehicle_len, double vehicle_wid, int32_t k, const int32_t* nbr, const double* w, int32_t B,
                     const double* start, const double* goal, uint8_t* found, double* cost, int32_t* seq,
                     int32_t* seq_len, int32_t* settled, uint8_t* direct_free);

/* ---------------------------------------------------------- diagnostics */
/* Evaluate one include/mp_jlmath.h function on the device for n inputs
 * (bit-exactness check against the CPU build).  fn: 0 sin, 1 cos, 2 tan, 3 atan,
 * 4 atan2(x, y), 5 asin, 6 acos, 7 exp, 8 log, 9 modpi, 10 sqrt; the branch-free
 * variants of the hot kernels: 11 modpi_bl, 12 atan_bl, 13 atan_tab, 14 sin (sincos_bl),
 * 15 cos (sincos_bl), 16 exp_fdlibm, 17 tan_bl, 18 atan2_sel(x, y), 19 sin / 20 cos (sincos_wide),
 * 21 tan_wide, 22 sin_34 (tyre sin, |x| <= 3π/4 fast path), 23 log_bl, 24 atan_rows — each must equal its
 * exact routine bit for bit.  The exact cheap divisions x / y, each equal to `/` bit for bit: 25 div_g
 * (guarded), 26 div_gn (hoisted reciprocal, divisor window checked by the caller), 27 div_gf (the same with
 * the fixup taking zero, Inf and NaN numerators), 28 / 29 the first / second quotient of the
 * shared-reciprocal pair div2_g (x, 1) / y and (-1.5, x) / y.  30: what v_div_scale_f64 does to x / y, as
 * 1·(numerator changed) + 2·(divisor changed) + 4·(VCC set), to check the guard's window against. */
int mp_math_eval(mp_ctx* ctx, int32_t fn, int64_t n, const double* x, const double* y, double* out);

/* Evaluate the 2x2 pseudo-inverse / SVD of include/mp_jlmath.h on the device for n row-major matrices
 * M[n][4], one thread per matrix in 256-thread blocks (bit-exactness check against the CPU build; n <= 2^24).
 * mode 0: mpj_pinv2 (exact, branchy)            -> out[n][4] = P;
 * mode 1: mpj_pinv2_bl (the Riccati sweep's)    -> out[n][4] = P.  Its exact fallback is taken by a whole
 *         wave when any of its lanes is rare, so matrix i meets the matrices 64*(i/64) .. 64*(i/64) + 63;
 * mode 2: mpj_pinv2_fast (straight-line path)   -> out[n][4] = P (meaningful where rare is 0), rare[i] = 0 / 1;
 * mode 3: mpj_svd2                              -> out[n][10] = U[4], S[2], VT[4].
 * rare[n] is optional (NULL to skip) and written as 0 in the modes other than 2. */
int mp_pinv2_eval(mp_ctx* ctx, int32_t mode, int64_t n, const double* M, double* out, int32_t* rare);

#ifdef __cplusplus
}
#endif
#endif /* MPGPU_H */
