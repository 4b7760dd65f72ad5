/*
 * usv_hip.h — C-ABI of libusvhip.so, the MI355X-native batched USV path-following
 * environment (usv-simple / usv-asmc-simple step on gfx950).
 *
 * Drop-in boundary.  The reference (romi2002/gym-usv) is pure Python; its interface for
 * this path is the Gymnasium Env API of its env classes, driven N-at-a-time by SB3's
 * DummyVecEnv (train_test/sb3_train_vec.py:67).  Each entry point below replaces:
 *
 *   usv_create      <- gymnasium.make(env_id) x N / UsvSimpleEnv.__init__
 *                      (gym_usv/__init__.py:24-34, gym_usv/envs/simple_env.py:10-60,
 *                       gym_usv/envs/simple_env_asmc.py:10-12)
 *   usv_seed        <- Env.reset(seed=...) seeding of np_random (simple_env.py:229)
 *   usv_reset       <- UsvSimpleEnv.reset (simple_env.py:228-308),
 *                      UsvSimpleASMCEnv.reset (simple_env_asmc.py:14-16),
 *                      UsvAsmcEnv.reset (usv_asmc_env.py:258-300),
 *                      UsvAsmcYeIntEnv.reset (usv_asmc_ye_int_env.py:256-296),
 *                      UsvPidEnv.reset (usv_pid_env.py:236-276)
 *   usv_reset_ex    <- UsvSimpleEnv.reset(options={'place_obstacles_on_path': k}) (:276-288) and
 *                      its info dict _get_info(-1, zeros(3)) (simple_env.py:102-115, :305)
 *   usv_set_experiment <- UsvSimpleEnv(options={'run_custom_experiment': ..}) (:10, :292-300)
 *   usv_set_ignore_obstacles <- the attribute UsvSimpleEnv.ignore_obstacles (simple_env.py:49,
 *                      read at :155, :222-224, :334)
 *   usv_step_ex     <- the step's info dict (simple_env.py:102-115, 189-199, 343-344)
 *   usv_step        <- UsvSimpleEnv.step (simple_env.py:310-346),
 *                      UsvSimpleASMCEnv.step (simple_env_asmc.py:18-27) -> UsvAsmc.compute
 *                      (gym_usv/control/usv_asmc.py:53-244), lidar
 *                      (gym_usv/envs/usv_asmc_ca_env.py:411-461,500-519), TimeLimit
 *                      (gym_usv/__init__.py:27,33) and DummyVecEnv same-step autoreset;
 *                      legacy UsvAsmcEnv.step (usv_asmc_env.py:99-255, compute_reward :364-374),
 *                      UsvAsmcYeIntEnv.step (usv_asmc_ye_int_env.py:92-253, :350-360),
 *                      UsvPidEnv.step (usv_pid_env.py:89-233, :329-338)
 *   usv_asmc_compute <- UsvAsmc.compute (gym_usv/control/usv_asmc.py:53-244), the controller
 *                      on its own, as the reference's tests drive it (tests/test_usv_asmc.py:8-37)
 *   usv_wrap_step / usv_wrap_reset <- VecFrameStack(env, 5) (train_test/sb3_train_vec.py:70; SB3
 *                      StackedObservations), gym.wrappers.RecordEpisodeStatistics (:43) and the
 *                      Monitor make_vec_env puts on each env (:67)
 *   usv_get_field / usv_set_field / usv_get_state / usv_set_state
 *                   <- the env attributes (position, velocity, obstacle_positions, ...);
 *                      used for checkpointing and for parity state injection
 *
 * Conventions: plain pointers and sizes, no torch / HIP types.  `stream` is a hipStream_t
 * passed as void* (NULL = default stream).  Device pointers (`*_dev`) are caller-owned
 * device memory (e.g. torch tensors' data_ptr()).  Launches are asynchronous and
 * stream-ordered.  Every function returns 0 on success or a negative usv_status; the
 * message is in usv_last_error() (thread-local).  A handle is not thread-safe; use one
 * handle per device (one process per GPU).
 */
#ifndef USV_HIP_H
#define USV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define USV_ABI_VERSION 5
#define USV_SENSOR_COUNT 128
#define USV_OBS_DIM 143      /* 15 + 128, simple_env.py:27 */
#define USV_ACT_DIM 2        /* simple_env.py:30 */
#define USV_ASMC_STATE 16    /* unique UsvAsmc state values (usv_asmc.py:43-49) */

typedef enum usv_status {
  USV_OK = 0,
  USV_ERR_ARG = -1,
  USV_ERR_HIP = -2,
  USV_ERR_ABI = -3,
  USV_ERR_STATE = -4
} usv_status;

typedef enum usv_mode {
  USV_MODE_SIMPLE = 0,       /* id "usv-simple"      (UsvSimpleEnv)                      */
  USV_MODE_ASMC_SIMPLE = 1,  /* id "usv-asmc-simple" (UsvSimpleASMCEnv)                  */
  USV_MODE_ASMC_V0 = 2,      /* id "usv-asmc-v0" legacy UsvAsmcEnv (usv_asmc_env.py:14): */
                             /* obs 6, scalar action, no lidar, no TimeLimit             */
  USV_MODE_ASMC_YE_INT_V0 = 3, /* id "usv-asmc-ye-int-v0" UsvAsmcYeIntEnv               */
                               /* (usv_asmc_ye_int_env.py:14): float64, ye integral      */
  USV_MODE_PID_V0 = 4          /* id "usv-pid-v0" UsvPidEnv (usv_pid_env.py:14): float64 */
} usv_mode;

typedef enum usv_precision { USV_F32 = 0, USV_F64 = 1 } usv_precision;

typedef enum usv_autoreset {
  USV_AUTORESET_SAME_STEP = 0, /* done envs reset inside usv_step (SB3 DummyVecEnv) */
  USV_AUTORESET_DISABLED = 1   /* done envs keep stepping until usv_reset(mask)       */
} usv_autoreset;

typedef enum usv_reset_rng {
  USV_RESET_PHILOX = 0,      /* Philox4x32-10 keyed by (seed, global env id, episode): the
                                reference's reset distributions, not its streams (default)   */
  USV_RESET_NUMPY_PCG64 = 1  /* each env's own numpy Generator(PCG64) (USV_FIELD_NP_RNG), drawn
                                in the reference's order: resets equal the reference's; the
                                legacy *-v0 ids draw from np.random's MT19937 (USV_FIELD_NP_MT) */
} usv_reset_rng;

typedef enum usv_lidar_algo {
  USV_LIDAR_BRUTE = 0,  /* every (ray, obstacle) pair                         */
  USV_LIDAR_WINDOW = 1  /* angular-window pruning, bit-identical to BRUTE    */
} usv_lidar_algo;

typedef struct usv_config {
  int32_t abi_version;       /* must be USV_ABI_VERSION */
  int32_t mode;              /* usv_mode */
  int32_t precision;         /* usv_precision: state + arithmetic type; obs is always f32 */
  int32_t num_envs;          /* envs owned by this handle */
  int32_t obstacle_cap;      /* max obstacles per env (reference draws 15..29) */
  int32_t max_episode_steps; /* TimeLimit; 0 = none. 500 usv-simple, 1000 usv-asmc-simple */
  int32_t autoreset;         /* usv_autoreset */
  int32_t lidar_algo;        /* usv_lidar_algo */
  uint64_t seed;             /* Philox key for in-kernel resets */
  uint64_t env_id_offset;    /* global id of env 0 (sharding across GPUs) */
  int32_t flags;             /* usv_flags */
  int32_t reserved;          /* 0 */
} usv_config;

typedef enum usv_flags {
  /* usv-asmc-simple: UsvAsmc.compute(..., do_perturb=True) (gym_usv/control/usv_asmc.py:184-199):
     a sinusoidal force is added to the thrust every substep; the controller's perturb_step is
     20 * elapsed + substep (a fresh UsvAsmc per episode, 2 x 10 substeps per env step) */
  USV_FLAG_PERTURB = 1,
  /* usv-simple / usv-asmc-simple: UsvSimpleEnv.ignore_obstacles (gym_usv/envs/simple_env.py:49) set
     from the start; usv_set_ignore_obstacles toggles it later.  USV_ERR_ARG for the legacy *-v0 ids,
     which have no obstacles. */
  USV_FLAG_IGNORE_OBSTACLES = 2
} usv_flags;

/* Per-step info (opt-in, usv_step_ex / usv_reset_ex): one row of USV_INFO_DIM values per env, in the
 * handle's precision (f32, or f64 for USV_F64: usv_reward_bytes gives the element size),
 * the keys of UsvSimpleEnv._get_info + reward_info (gym_usv/envs/simple_env.py:102-115,189-199).
 * "reward" is rew_dev itself; keys that are constant in the reference (left/right_thruster = 0,
 * angle_action_reward = 0) are not stored.  After an explicit reset the row is
 * _get_info(-1, zeros(3)) (:305): the reward-term entries are 0.  With same-step autoreset the
 * row of a done env keeps its terminal step's info. */
typedef enum usv_info_key {
  USV_INFO_X = 0, USV_INFO_Y, USV_INFO_PSI,      /* 'position' (after the step)            */
  USV_INFO_U, USV_INFO_V, USV_INFO_R,            /* 'velocity'                             */
  USV_INFO_PATH_X0, USV_INFO_PATH_Y0,            /* 'path_start'                           */
  USV_INFO_PATH_X1, USV_INFO_PATH_Y1,            /* 'path_end'                             */
  USV_INFO_ACTION0, USV_INFO_ACTION1,            /* 'action0', 'action1' (filtered action)  */
  USV_INFO_YE,                                   /* 'ye'                                   */
  USV_INFO_ANGLE_TO_TARGET,                      /* 'angle_to_target' (= angle / pi)       */
  USV_INFO_YE_REWARD, USV_INFO_ANGLE_TO_TARGET_REWARD, USV_INFO_DELTA_ACTION_REWARD,
  USV_INFO_DELTA_ACTION, USV_INFO_VELOCITY_TRACK_REWARD,
  USV_INFO_REFERENCE_VELOCITY, USV_INFO_REWARD_VELOCITY, USV_INFO_REFERENCE_VELOCITY_ERROR,
  USV_INFO_DIM
} usv_info_key;

/* reset(options=...) of UsvSimpleEnv.reset (simple_env.py:276-288) */
typedef struct usv_reset_options {
  int32_t place_obstacles_on_path;  /* k > 0: k extra obstacles scattered along the path;
                                       needs obstacle_cap >= 29 + k */
  int32_t reserved;
} usv_reset_options;

/* __init__(options={'run_custom_experiment': True, 'experiment': {...}}) of UsvSimpleEnv
 * (simple_env.py:10,292-300): every reset (explicit or autoreset) of every env of the handle
 * replaces the drawn obstacles, path and pose by these, after the usual draws. */
typedef struct usv_experiment {
  int32_t n_obs;               /* 1 .. obstacle_cap */
  int32_t reserved;
  double obstacle_x[64], obstacle_y[64], obstacle_r[64];  /* 'obstacle_positions', 'obstacle_radius' */
  double path_start[2];        /* 'path_start' */
  double angle;                /* 'angle': path_end = path_start + (cos, sin)(angle) * 100 */
  double position[3];          /* 'position' (x, y, psi) */
} usv_experiment;

/* Per-env state fields.  Host-side layout for get/set: [num_envs][per_env] row-major,
 * float64 for real fields, int32 for integer fields (usv_field_info tells which). */
typedef enum usv_field {
  USV_FIELD_X = 0, USV_FIELD_Y, USV_FIELD_PSI,          /* position (simple_env.py:39) */
  USV_FIELD_U, USV_FIELD_V, USV_FIELD_R,                /* velocity (:38)              */
  USV_FIELD_LAST_U, USV_FIELD_LAST_R,                   /* last_action[0], [2] (:41)   */
  USV_FIELD_PROGRESS,                                   /* progress (:53)              */
  USV_FIELD_PATH_X0, USV_FIELD_PATH_Y0,                 /* path_start (:51)            */
  USV_FIELD_PATH_X1, USV_FIELD_PATH_Y1,                 /* path_end (:52)              */
  USV_FIELD_MAX_U, USV_FIELD_MAX_R,                     /* max_action[0], [2] (:32)    */
  USV_FIELD_REF_V,                                      /* reference_velocity (:33)    */
  USV_FIELD_N_OBS,          /* int: obstacle_n (:44)                                    */
  USV_FIELD_ELAPSED,        /* int: TimeLimit elapsed steps                              */
  USV_FIELD_EPISODE,        /* int: episode counter (Philox counter word)                */
  USV_FIELD_SCAN_VALID,     /* int: 1 if the current pose's scan is the stale sensor_data; 2 if the
                               stale sensor_data is all max range (last step ignored the obstacles) */
  USV_FIELD_OBS_X, USV_FIELD_OBS_Y, USV_FIELD_OBS_R,    /* [cap] obstacles (:45-46)    */
  USV_FIELD_SENSOR_LAST,    /* [128] stale scan for reset obs (sensor_data, :47)          */
  USV_FIELD_ASMC,           /* [16] UsvAsmc state (usv-asmc-simple only)                  */
  USV_FIELD_V0_LAST,        /* [9]  usv-asmc-v0 `last` (eta_dot, upsilon_dot, e_u_last, Ka_dots) */
  USV_FIELD_V0_AUX,         /* [3]  usv-asmc-v0 `aux_vars` (e_u_int, Ka_u, Ka_psi)        */
  USV_FIELD_V0_TARGET,      /* [6]  usv-asmc-v0 `target` (x_0, y_0, speed, ak, x_d, y_d)  */
  USV_FIELD_V0_ACTION_LAST, /* [1]  usv-asmc-v0 state[5] (previous action)                 */
  USV_FIELD_V0_YE,          /* [2]  usv-asmc-ye-int-v0 aux_vars[3] ye_int, last[9] ye_last  */
  USV_FIELD_NP_RNG,         /* int [10]: the env's numpy Generator(PCG64) for USV_RESET_NUMPY_PCG64:
                               state high / low and increment high / low 64-bit words as
                               little-endian 32-bit halves, has_uint32, uinteger
                               (bit_generator.state of np.random.PCG64)                    */
  USV_FIELD_NP_MT,          /* int [625] (legacy *-v0 ids; 0 otherwise): np.random's global
                               RandomState MT19937 key[624] and pos, for USV_RESET_NUMPY_PCG64 */
  USV_FIELD_COUNT
} usv_field;

int usv_abi_version(void);
const char* usv_last_error(void);
/* sizeof(usv_config) as compiled into the library (56): a binding checks its own struct against it
 * (ABI v5). */
size_t usv_config_size(void);

/* Fill `cfg` with the reference defaults for `mode` (cap 32, TimeLimit by id -- 500, 1000,
 * none for the legacy *-v0 ids --, f32, same-step autoreset, window lidar, seed 0). */
void usv_config_default(usv_config* cfg, int32_t mode, int32_t num_envs);

int usv_create(const usv_config* cfg, int32_t device, void** handle_out);
void usv_destroy(void* handle);

int usv_num_envs(void* handle);
int usv_obs_dim(void* handle);   /* 143 (usv-simple, usv-asmc-simple) or 6 (legacy *-v0 ids) */
int usv_act_dim(void* handle);   /* 2, or 1 for the legacy *-v0 ids */
/* Bytes of one reward element (4 for USV_F32, 8 for USV_F64). */
int usv_reward_bytes(void* handle);

/* Re-key the reset RNG (Philox4x32-10, key = seed, counter = global env id / episode)
 * and zero every episode counter.  Host-side only; no launch. */
int usv_seed(void* handle, uint64_t seed);

/* Select the reset RNG (usv_reset_rng) <- Env.reset(seed) seeding np_random
 * (simple_env.py:229, gymnasium seeding.np_random) and np.random.seed + np.random.uniform
 * (usv_asmc_env.py:258-279).  The generator states are set through USV_FIELD_NP_RNG /
 * USV_FIELD_NP_MT. */
int usv_set_reset_rng(void* handle, int32_t kind);

/* Reset envs whose mask byte is non-zero (all envs if mask_dev == NULL) and write their
 * reset observation rows into obs_dev [num_envs][obs_dim] (other rows untouched). */
int usv_reset(void* handle, const uint8_t* mask_dev, float* obs_dev, void* stream);
/* usv_reset with reset options (NULL = none) and an optional info buffer info_dev
 * [num_envs][USV_INFO_DIM] f32 / f64 by precision (NULL = none; rows of reset envs are written). */
int usv_reset_ex(void* handle, const uint8_t* mask_dev, float* obs_dev,
                 const usv_reset_options* options, void* info_dev, void* stream);
/* Install (experiment != NULL) or remove (NULL) the custom experiment of every env. */
int usv_set_experiment(void* handle, const usv_experiment* experiment);

/* One env step for every env.
 *   act_dev       [num_envs][act_dim] f32 (u in [0.2,1], r in [-1,1]; usv-asmc-simple: (u_d, psi
 *                 offset); legacy *-v0 ids: heading offset in [-pi/2, pi/2])
 *   obs_dev       [num_envs][obs_dim] f32  (reset obs for envs that autoreset)
 *   rew_dev       [num_envs] f32 or f64 (usv_reward_bytes)
 *   term_dev, trunc_dev [num_envs] u8
 *   final_obs_dev [num_envs][obs_dim] f32 or NULL: terminal obs rows of done envs
 *                 (rows of envs not done are left untouched). */
int usv_step(void* handle, const float* act_dev, float* obs_dev, void* rew_dev,
             uint8_t* term_dev, uint8_t* trunc_dev, float* final_obs_dev, void* stream);
/* usv_step with two optional outputs (NULL = not written):
 *   done_dev  [num_envs] u8: terminated | truncated, i.e. gymnasium's info['_final_obs'] mask (ABI v4)
 *   info_dev  [num_envs][USV_INFO_DIM] f32 / f64 by precision: the per-step info rows (usv-simple /
 *             usv-asmc-simple; the legacy *-v0 ids return {} in the reference and ignore it). */
int usv_step_ex(void* handle, const float* act_dev, float* obs_dev, void* rew_dev,
                uint8_t* term_dev, uint8_t* trunc_dev, uint8_t* done_dev, float* final_obs_dev,
                void* info_dev, void* stream);

/* UsvAsmc.compute(action, position, velocity, do_perturb) (gym_usv/control/usv_asmc.py:53-244) for
 * n independent controllers, `calls` compute() calls back to back (10 substeps of 0.01 s each), in
 * place on device buffers of the precision's type (float for USV_F32, double for USV_F64):
 *   act_dev [n][2] (u_d, heading offset), pos_dev [n][3] (x, y, psi), vel_dev [n][3] (u, v, r),
 *   state_dev [16][n]: psi_d_last, o, o', o'', eta_dot_last[3], upsilon_dot_last[3], e_u_last,
 *     Ka_dot_u_last, Ka_dot_psi_last, e_u_int, Ka_u, Ka_psi (so_filter / last / aux_vars, :43-49;
 *     the reference keeps so_filter's o_last, o_dot_last, o_dot_dot_last equal to o, o', o'');
 *   perturb_step_dev int32 [n] or NULL (= 0): the controllers' perturb_step (:49), advanced by 10
 *     per call; do_perturb adds the sinusoidal disturbance (:184-199).
 * Stream-ordered, no handle (ABI v5); launched on the device that holds state_dev, whatever device is
 * current (USV_ERR_ARG if any buffer is not device memory of the device that holds state_dev). */
int usv_asmc_compute(int32_t precision, int32_t n, const void* act_dev, void* pos_dev, void* vel_dev,
                     void* state_dev, int32_t* perturb_step_dev, int32_t do_perturb, int32_t calls,
                     void* stream);

/* Fused training wrappers: the two wrappers the reference's training setup puts on every env, for all
 * envs in one launch behind usv_step on the same stream, with no host sync:
 *   usv_wrap_step  <- VecFrameStack(env, 5) (train_test/sb3_train_vec.py:70), i.e. SB3
 *                     StackedObservations.update (channels-last: roll by one obs, a done env's stack
 *                     zeroed, the new obs pushed; terminal_observation = the old stack rolled, with the
 *                     final obs as its last frame), and RecordEpisodeStatistics (:43) / SB3 Monitor
 *                     (make_vec_env wraps every env in one, :67): episode return and length, emitted
 *                     and restarted when the env is done
 *   usv_wrap_reset <- StackedObservations.reset (zeros, the reset obs last) and Monitor.reset
 * Handle-free and stream-ordered like usv_asmc_compute (ABI v5 addition); launched on the device that
 * holds `ring`.  The stack is a mirrored ring, never shifted: per env one row of
 * usv_wrap_ring_stride(obs_dim, n_stack) floats (2 n_stack - 1 slots of obs_dim floats, rounded up to 4
 * floats).  The caller counts steps: j is the index of the frame being written, the same for every env,
 * j >= 0, and successive steps pass j, j + 1, ...  After the call with j, the stacked observation of env
 * e is the n_stack * obs_dim floats at ring + e * stride + usv_wrap_window_offset(obs_dim, n_stack, j),
 * oldest frame first: for all envs one [n][n_stack * obs_dim] view with row stride `stride`, valid until
 * the next call.  n_stack = 1 keeps the statistics only (the ring is then a copy of obs).
 *
 * usv_wrap_step, per env, in this order:
 *   ep_ret += reward (f64; the reward read as f32 or f64 by reward_bytes), ep_len += 1;
 *   if done_dev[e]: final_stack_dev[e] = (frames j-n_stack+1 .. j-1, final_obs_dev[e]) unless NULL;
 *     episode[e] = (ep_ret, ep_len); cum_ret[e] += ep_ret, cum_len[e] += ep_len, cum_eps[e] += 1;
 *     ep_ret = ep_len = 0; the frames before j become zero;
 *   frame j = obs_dev[e].
 * Rows of final_stack_dev and episode of envs that are not done are left untouched.  No atomics: the
 * interval totals are cum_*.sum(), taken by the caller when it reports.
 * "Become zero": +0.0 is stored, as StackedObservations' `stacked_obs[i] = 0` does.  With
 * USV_WRAP_CLEAR_KEEPS_SIGN in `flags` the step multiplies those frames by zero instead, which keeps
 * each value's sign (-0.0 where the frame was negative): what a stack cleared by a mask multiply
 * holds, as the default path of gym_usv_amd.sb3.Sb3VecEnv clears it, so that the fused adapter equals
 * that path bit for bit.  The two differ only in the sign of zeros, which a later terminal stack shows.
 * usv_wrap_reset, for envs whose mask byte is non-zero (all if mask_dev == NULL): the frames before j
 * become zero, frame j = obs_dev[e], ep_ret = ep_len = 0 (cum_* are the caller's to zero).
 *
 * USV_ERR_ARG, before any HIP call, for n <= 0, obs_dim <= 0, n_stack < 1, a NULL ring, j < 0,
 * reward_bytes not 4 / 8 or an unknown flag; then for a missing buffer, one not aligned to its element size (obs rows and
 * the ring need 4-B alignment only) or not device memory of the ring's device. */
typedef enum usv_wrap_flags { USV_WRAP_CLEAR_KEEPS_SIGN = 1 } usv_wrap_flags;
typedef struct usv_wrap {      /* caller-owned device buffers */
  int32_t n, obs_dim, n_stack, reward_bytes;
  int32_t flags;               /* usv_wrap_flags */
  int32_t reserved;            /* 0 */
  float* ring;                 /* [n][usv_wrap_ring_stride] */
  double* ep_ret;              /* [n] running episode return */
  int32_t* ep_len;             /* [n] running episode length */
  double* episode;             /* [n][2] (r, l), rows of done envs written; may be NULL */
  double* cum_ret;             /* [n] sums over the emitted episodes; the three may be NULL together */
  int64_t* cum_len;
  int64_t* cum_eps;
} usv_wrap;
size_t usv_wrap_ring_stride(int32_t obs_dim, int32_t n_stack);   /* floats per env row; host only; 0 if bad */
size_t usv_wrap_window_offset(int32_t obs_dim, int32_t n_stack, int64_t j);   /* floats; host only */
int usv_wrap_reset(const usv_wrap* w, int64_t j, const uint8_t* mask_dev, const float* obs_dev, void* stream);
int usv_wrap_step(const usv_wrap* w, int64_t j, const float* obs_dev, const void* rew_dev,
                  const uint8_t* done_dev, const float* final_obs_dev, float* final_stack_dev, void* stream);

/* Fused VecNormalize: SB3's VecNormalize (stable_baselines3/common/vec_env/vec_normalize.py) between the
 * step and the frame stack, VecFrameStack(VecNormalize(venv)), for all envs behind usv_step on the same
 * stream with no host sync.  Additive and handle-free like usv_wrap_* (ABI v5 addition).  usv_norm holds
 * the caller-owned statistics; start them as RunningMeanStd.__init__ does: mean = 0, var = 1,
 * count = 1e-4 (running_mean_std.py), returns = 0.
 *
 * usv_wrap_step_norm = usv_wrap_step with, in this order (flags: T = USV_NORM_TRAINING, O = USV_NORM_OBS,
 * R = USV_NORM_REWARD):
 *   1. T and O: obs_rms.update(obs_dev), per column of the [n][obs_dim] obs the step wrote (a done env's
 *      row is its reset obs, as in DummyVecEnv)                    <- step_wait: self.obs_rms.update(obs)
 *   2. T and R: returns = returns * gamma + reward in f64, then ret_rms.update(returns)
 *                                                                  <- step_wait: _update_reward
 *   update = RunningMeanStd.update_from_moments with the batch mean, population variance and count n:
 *     delta = bm - mean; tot = count + n; mean += delta n / tot;
 *     M2 = var count + bv n + delta^2 count n / tot; var = M2 / tot; count = tot.
 *   3. obs_inv_std[c] = 1 / sqrt(obs_var[c] + epsilon), ret_inv_std = 1 / sqrt(ret_var + epsilon) are
 *      published (f64), from the statistics as they stand after 1 and 2 (or as stored, with T off)
 *   4. frame j = float(clamp((double(obs) - obs_mean[c]) * obs_inv_std[c], -clip_obs, clip_obs)) with O,
 *      the raw obs without                                         <- normalize_obs
 *   5. the final obs of a done env is transformed like 4 before it becomes the last frame of
 *      final_stack; the older frames are the ring's, normalised when they were pushed
 *   6. norm_rew_out[e] = float(clamp(double(reward) * ret_inv_std, -clip_reward, clip_reward)) with R
 *      (no mean is subtracted), float(reward) without              <- normalize_reward
 *   7. returns[e] = 0 for done envs                                <- step_wait: self.returns[dones] = 0
 *   8. ep_ret, episode and cum_* use the raw reward (the Monitor sits inside VecNormalize); the clear of a
 *      done env's stack and the ring layout are usv_wrap_step's.
 * Deviation from SB3: 4 to 6 multiply by the published reciprocal where SB3 divides by
 * sqrt(var + epsilon); the value before the rounding to f32 differs by at most one f64 ulp.  In return
 * the outputs are a bit-exact function of the published obs_mean / obs_inv_std / ret_inv_std:
 * ((x.astype(f64) - mean) * inv).clip(-c, c).astype(f32) in NumPy gives the same bits.
 * The batch moments are accumulated as (count, mean, M2) in f64, combined in a fixed order (no atomics):
 * two calls on the same input give the same bits.  With T on (and O or R) the call is three launches
 * (partial moments, finalise, normalising step), otherwise one.
 *
 * usv_wrap_reset_norm = usv_wrap_reset with returns = 0 for the restarted envs and frame j normalised.
 * mask_dev == NULL (VecNormalize.reset): with T and O the statistics are first updated with obs_dev.
 * A masked reset (no SB3 counterpart) updates no statistic and uses the current ones.
 * The statistics are per process: no collective is involved (a multi-GPU run keeps one set per rank).
 *
 * USV_ERR_ARG as for usv_wrap_*, and before any HIP call for a NULL usv_norm, n / obs_dim <= 0 or not
 * the usv_wrap's, obs_dim > 4096, unknown flags, a negative (or NaN) clip, gamma outside [0, 1],
 * epsilon <= 0, a NULL buffer or one not 8-B aligned; then for a buffer that is not device memory of the
 * ring's device.  scratch needs usv_norm_scratch_bytes(n, obs_dim) bytes and is overwritten by every
 * updating call. */
typedef enum usv_norm_flags { USV_NORM_TRAINING = 1, USV_NORM_OBS = 2, USV_NORM_REWARD = 4 } usv_norm_flags;
typedef struct usv_norm {      /* caller-owned device buffers, all f64 */
  int32_t n, obs_dim;
  int32_t flags;               /* usv_norm_flags */
  int32_t reserved;            /* 0 */
  double clip_obs, clip_reward, gamma, epsilon;   /* SB3 defaults: 10, 10, 0.99, 1e-8 */
  double* obs_mean;            /* [obs_dim] */
  double* obs_var;             /* [obs_dim] */
  double* obs_inv_std;         /* [obs_dim], written by every call */
  double* obs_count;           /* [1] */
  double* ret_mean;            /* [1] (kept as RunningMeanStd keeps it; not used by the transform) */
  double* ret_var;             /* [1] */
  double* ret_inv_std;         /* [1], written by every call */
  double* ret_count;           /* [1] */
  double* returns;             /* [n] discounted return per env */
  double* scratch;             /* usv_norm_scratch_bytes(n, obs_dim) */
} usv_norm;
size_t usv_norm_scratch_bytes(int32_t n, int32_t obs_dim);   /* host only; 0 if bad */
int usv_wrap_step_norm(const usv_wrap* w, const usv_norm* z, int64_t j, const float* obs_dev, const void* rew_dev,
                       const uint8_t* done_dev, const float* final_obs_dev, float* final_stack_dev,
                       float* norm_rew_out_dev, void* stream);
int usv_wrap_reset_norm(const usv_wrap* w, const usv_norm* z, int64_t j, const uint8_t* mask_dev,
                        const float* obs_dev, void* stream);

/* Device rollout buffer: SB3's RolloutBuffer (stable_baselines3/common/buffers.py) and the truncation
 * bootstrap of OnPolicyAlgorithm.collect_rollouts (common/on_policy_algorithm.py) behind usv_step and
 * usv_wrap_step on the same stream, with no host sync between a rollout's first action and its advantages.
 * Additive, handle-free and stream-ordered like usv_wrap_* (ABI v5 addition); launched on the device that
 * holds `obs`.  All buffer arithmetic is float32, every operation rounded on its own (no FMA), as NumPy
 * computes it; tests/rollout_ref.py restates it and the kernels equal it bit for bit.
 *
 * A rollout is n_steps = T steps of n envs whose stored observation rows are obs_width = W floats.
 *
 * usv_rollout_put_obs(ro, t, ...), before the env step t (the wrappers' next push overwrites the oldest
 * frame of the window it reads):                            <- RolloutBuffer.add
 *   obs[t] = obs_src rows (any 4-B-aligned base, row stride >= W floats: DeviceWrappers.stacked, the
 *            ring's window with row stride usv_wrap_ring_stride, is read in place, without a clone);
 *   act[t] = act_dev [n][act_dim] (the unclipped action), val[t] = val_dev [n], logp[t] = logp_dev [n].
 * usv_rollout_put_step(ro, t, ...), after the env step t:
 *   rew[t] = float32(reward) (read as f32 or f64 by reward_bytes)   <- add: self.rewards[pos] = reward
 *   start[t + 1] = terminated | truncated                           <- collect_rollouts:
 *                                                                      self._last_episode_starts = dones
 *   an env with truncated and not terminated (the adapter's TimeLimit.truncated) takes a terminal slot s
 *   and term_obs[s] = its row of final_stack_dev [n][W] (usv_wrap_step's final_stack, or the step's final
 *   obs without a stack); term_slot[t][e] = s, and -1 for every other env
 *                                                    <- collect_rollouts: infos[idx]["terminal_observation"]
 *   Slots are deterministic: s is the number of such (t', e') pairs earlier in (t, env) order within the
 *   rollout.  t == 0 restarts the numbering.  A pair whose number is >= term_cap gets -1 and no bootstrap;
 *   term_count = (pairs stored, pairs dropped) after every call.  Calls of one rollout pass t = 0, 1, ...
 * usv_rollout_gae(ro, last_val_dev [n], term_val_dev [term_cap], gamma, gae_lambda), after step T - 1, with
 *   term_val[s] = the caller's V(term_obs[s]) and g32 = float32(gamma), gl32 = float32(gamma * gae_lambda):
 *   for t = T - 1 .. 0, gae = 0 at the start:               <- compute_returns_and_advantage
 *     r     = rew[t], or rew[t] + g32 * term_val[term_slot[t]] where the slot is >= 0
 *                                                    <- collect_rollouts: rewards[idx] += gamma * terminal_value
 *     nnt   = 1 - start[t + 1];  nv = val[t + 1], last_val at t = T - 1
 *     delta = (r + ((g32 * nv) * nnt)) - val[t]
 *     gae   = delta + ((gl32 * nnt) * gae)
 *     adv[t] = gae;  ret[t] = adv[t] + val[t]
 *   then start[0] = start[T]: row T of one rollout is row 0 of the next (the caller starts the first
 *   rollout with start[0] = 1, SB3's _last_episode_starts = np.ones).  term_val is read only at slots that
 *   term_slot references.
 * Deviation from SB3: rew keeps the raw reward and the bootstrapped value lives inside the GAE only,
 * where SB3 adds it into buffer.rewards (which PPO never reads again); calling usv_rollout_gae twice
 * therefore gives the same bits.
 *
 * USV_ERR_ARG, before any HIP call, for a NULL usv_rollout, n / n_steps / obs_width / act_dim <= 0,
 * term_cap < 0, reserved != 0, t outside [0, n_steps), reward_bytes not 4 / 8, a row stride below
 * obs_width, gamma or gae_lambda outside [0, 1] (or NaN), a NULL buffer or one not aligned to its element
 * size (scratch: 8 B); term_obs, final_stack_dev and term_val_dev may be NULL only with term_cap == 0.
 * Then for a buffer that is not device memory of the device that holds obs.  scratch needs
 * usv_rollout_scratch_bytes(n) bytes and belongs to the rollout between put_step(0) and the gae. */
typedef struct usv_rollout {   /* caller-owned device buffers */
  int32_t n, n_steps, obs_width, act_dim;
  int32_t term_cap;            /* rows of term_obs */
  int32_t reserved;            /* 0 */
  float* obs;                  /* [T][n][W] */
  float* act;                  /* [T][n][act_dim] */
  float* rew;                  /* [T][n] */
  float* val;                  /* [T][n] */
  float* logp;                 /* [T][n] */
  float* adv;                  /* [T][n], written by usv_rollout_gae */
  float* ret;                  /* [T][n], written by usv_rollout_gae */
  uint8_t* start;              /* [T + 1][n] episode_starts */
  int32_t* term_slot;          /* [T][n] */
  float* term_obs;             /* [term_cap][W] */
  int32_t* term_count;         /* [2] (stored, overflow) */
  void* scratch;               /* usv_rollout_scratch_bytes(n) */
} usv_rollout;
size_t usv_rollout_scratch_bytes(int32_t n);   /* host only; 0 if bad */
int usv_rollout_put_obs(const usv_rollout* ro, int32_t t, const float* obs_src_dev, size_t obs_row_stride_floats,
                        const float* act_dev, const float* val_dev, const float* logp_dev, void* stream);
int usv_rollout_put_step(const usv_rollout* ro, int32_t t, const void* rew_dev, int32_t reward_bytes,
                         const uint8_t* term_dev, const uint8_t* trunc_dev, const float* final_stack_dev,
                         void* stream);
int usv_rollout_gae(const usv_rollout* ro, const float* last_val_dev, const float* term_val_dev, double gamma,
                    double gae_lambda, void* stream);

/* Frame-deduplicated obs storage and the minibatch gather: the other half of SB3's RolloutBuffer
 * (get / _get_samples) and a rollout that keeps one D-float frame per (step, env) where usv_rollout.obs
 * keeps the whole k-frame stack.  Additive (ABI v5 addition); usv_rollout is unchanged.
 *
 * frames is [n][T + k - 1][D] float32, env-major: row r of env e is the frame pushed at time r - (k - 1),
 * so the k frames of sample (t, e) are the k D contiguous floats from row t on.
 *
 * usv_rollout_put_obs_frames(ro, fr, t, ...) replaces usv_rollout_put_obs (same source contract; act, val
 * and logp are stored as there): at t = 0 the whole [k D] window goes to rows 0 .. k - 1 of each env, at
 * t > 0 its newest D columns go to row t + k - 1.  Precondition: from put_obs(0) to the last put_obs of
 * a rollout the windows evolve by the VecFrameStack rule with exactly the dones given to
 * usv_rollout_put_step (a window reset by hand inside a rollout is not supported).  ro->obs is not read;
 * usv_rollout_put_step and usv_rollout_gae still refuse a NULL obs and never touch it: point it at frames.
 *
 * usv_rollout_gather(ro, fr, idx_dev [B] int64, B, out...): for sample i = idx[b] = t * n + e, one launch
 * writes obs_out[b] = the stacked row [W] that full storage would hold in obs[t][e], bit for bit, and
 * act_out[b] [act_dim], val_out / logp_out / adv_out / ret_out [b] = act / val / logp / adv / ret at i.
 *   Slot j of the row (0 = oldest) is the frame of time u = t - (k - 1 - j), cleared if some s with
 *   max(u, 0) < s <= t has start[s][e] != 0; a cleared element is +0.0, or x * 0.0f (-0.0 where x was
 *   negative) with USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN, as usv_wrap's USV_WRAP_CLEAR_KEEPS_SIGN.
 *   fr->frames == NULL: full storage, the row is obs[i] (k * d must still equal obs_width; k = 1 will do).
 *   An idx outside [0, T n) is not dereferenced: its outputs are NaN and *bad_count is incremented (it
 *   is never reset by the library); the call still returns USV_OK.
 *
 * USV_ERR_ARG, before any HIP call, for a NULL struct, k < 1, d < 1, k > 32, k * d != obs_width, unknown
 * flags, B <= 0, a NULL idx, output or bad_count, usv_rollout_put_obs_frames with frames == NULL, and
 * everything usv_rollout_put_obs refuses. */
#define USV_ROLLOUT_FRAMES_CLEAR_KEEPS_SIGN 1
typedef struct usv_rollout_frames {
  int32_t k, d;                /* n_stack and floats per frame; k * d == obs_width */
  int32_t flags;               /* USV_ROLLOUT_FRAMES_* */
  float* frames;               /* [n][T + k - 1][d], or NULL: full storage (gather only) */
  int32_t* bad_count;          /* [1] indices the gather refused */
} usv_rollout_frames;
int usv_rollout_put_obs_frames(const usv_rollout* ro, const usv_rollout_frames* fr, int32_t t,
                               const float* obs_src_dev, size_t obs_row_stride_floats, const float* act_dev,
                               const float* val_dev, const float* logp_dev, void* stream);
int usv_rollout_gather(const usv_rollout* ro, const usv_rollout_frames* fr, const int64_t* idx_dev, int32_t B,
                       float* obs_out, float* act_out, float* val_out, float* logp_out, float* adv_out,
                       float* ret_out, void* stream);

/* The gather a HIP graph can replay: SB3's RolloutBuffer.get without a stored permutation.  Additive (ABI v5
 * addition).  Which minibatch a call reads is not an argument, which a graph would freeze, but a cursor block in
 * device memory: usv_rollout_cursor_bytes() bytes (16), 16-B aligned, uint32 epoch at byte 0 and uint32 batch at
 * byte 4, the rest reserved; the caller zeroes it once and may write the two words between calls.
 *
 * usv_rollout_gather_perm(ro, fr, cursor_dev, seed, B, idx_out, out...), two launches and no sync, copy or
 * allocation.  With M = n_steps * n: sample b < B of the call is i = perm_index(seed, epoch, M, batch * B + b), a
 * bijection of [0, M) for every (seed, epoch): a six-round Feistel network over the next power of two (at least 4)
 * with cycle walking, its round keys from Philox4x32-10 with key = seed and counter (epoch, "PERM", block, 0), a
 * counter that the gSDE, CAPS and reset streams of the same seed never use (gym-usv_amd/csrc/usv_rollout_perm_math.hpp
 * states it; tests/rollout_perm_ref.py restates it).  The outputs are usv_rollout_gather's at these indices, bit
 * for bit; idx_out [B] int64, if not NULL, receives the indices.  Then one thread moves the cursor on: batch + 1,
 * or (epoch + 1, 0) after the epoch's last minibatch; epoch wraps at 2^32.  M / B calls visit every sample once.
 * A batch word that is not below M / B is read as 0.
 *
 * USV_ERR_ARG, before any HIP call, for B that does not divide M, a NULL or misaligned cursor block, an output
 * that is the cursor block, a misaligned idx_out, and everything usv_rollout_gather refuses. */
size_t usv_rollout_cursor_bytes(void);
int usv_rollout_gather_perm(const usv_rollout* ro, const usv_rollout_frames* fr, void* cursor_dev, uint64_t seed,
                            int32_t B, int64_t* idx_out, float* obs_out, float* act_out, float* val_out,
                            float* logp_out, float* adv_out, float* ret_out, void* stream);

/* Fused gSDE action head: SB3's StateDependentNoiseDistribution (common/distributions.py; full_std, no
 * expln, latent not learned through the noise) at rollout time, with the per-env exploration matrix rebuilt
 * from a counter-based generator in the launch that uses it instead of being stored.  Handle-free and
 * stream-ordered like usv_wrap_* and usv_rollout_*; additive (ABI v5 addition).  No host sync.
 *
 * The matrix (replaces sample_weights: exploration_mat = Normal(0, std).rsample((n,))).  Element (j, k) of
 * env e's [latent_dim][act_dim] matrix, flat index i = j * act_dim + k, is std[j][k] * z where z is normal
 * number i % 4 of Philox4x32-10 block i / 4 with key (seed lo, seed hi) and counter (gid lo, gid hi, epoch,
 * block), gid = gid0 + e.  A block's words (o0, o1, o2, o3) give z0 = r cos(2 pi u2), z1 = r sin(2 pi u2)
 * with u1 = ((o0 >> 8) + 1) * 2^-24, u2 = (o1 >> 8) * 2^-24, r = sqrt(-2 ln u1), and z2, z3 from (o2, o3)
 * the same way.  A new epoch is a new matrix (reset_noise: the caller increments it); the matrix does not
 * depend on n or on how envs are sharded (gid0 = the shard's first global env id).  Use a seed other than
 * the env's: the resets draw from the same generator keyed by usv_config.seed, counter (gid, episode, draw).
 *
 * usv_sde_sample(s, epoch, mean [n][A], lat [n] rows of latent_dim floats, row stride in floats, std
 * [latent_dim][A] = exp(log_std), act [n][A], act_env [n][A], logp [n]), all float32, one launch:
 *   noise_k = sum_j lat_j * (std_jk * z_jk)               <- get_noise: bmm(latent_sde, exploration_matrices)
 *   act_k   = mean_k + noise_k                            <- sample: mean + noise (unclipped: the buffer's)
 *   act_env_k = max(min(act_k, high_k), low_k)            <- the trainer's np.clip to the Box
 *   var_k   = sum_j (lat_j lat_j) (std_jk std_jk);  s2_k = var_k + 1e-6
 *                                                         <- proba_distribution: mm(latent_sde ** 2, std ** 2)
 *   logp    = sum_k (-(act_k - mean_k)^2 / (2 s2_k) - 0.5 ln s2_k - 0.5 ln 2 pi)
 *                                                         <- log_prob: Normal(mean, sqrt(s2)).log_prob(a).sum(-1)
 * in the operation and summation order of csrc/usv_sde_math.hpp.  The matrix is never written to memory.
 * usv_sde_weights(s, epoch, std, w [n][latent_dim][A]) writes the matrix itself (exploration_mat), from the
 * same device functions: for inspection, tests and checkpoints.
 *
 * USV_ERR_ARG, before any HIP call, for a NULL usv_sde, n <= 0, act_dim not 1 or 2, latent_dim outside
 * [4, 4096] or not a multiple of 4, reserved != 0, low[k] > high[k] or a NaN bound (k < act_dim), a row
 * stride below latent_dim or not a multiple of 4, a NULL buffer, a lat_dev that is not 16-B aligned or
 * another buffer that is not 4-B aligned, and a usv_sde_weights of more than 2^31 - 1 blocks of 256
 * four-element groups.  Then for a buffer that is not device memory of the device that holds lat_dev
 * (usv_sde_weights: w_dev). */
typedef struct usv_sde {
  int32_t n, latent_dim, act_dim, reserved;   /* reserved = 0 */
  uint64_t seed, gid0;
  float low[4], high[4];                      /* Box bounds, first act_dim used */
} usv_sde;
int usv_sde_sample(const usv_sde* s, uint32_t epoch, const float* mean_dev, const float* lat_dev,
                   size_t lat_row_stride_floats, const float* std_dev, float* act_dev, float* act_env_dev,
                   float* logp_dev, void* stream);
int usv_sde_weights(const usv_sde* s, uint32_t epoch, const float* std_dev, float* w_dev, void* stream);

/* The squashed, differentiable head: SAC's StateDependentNoiseDistribution(squash_output=True,
 * learn_features=True) with its backward.  The same usv_sde (reserved = 0), the same matrix and the same
 * noise_k and var_k as usv_sde_sample; additive (ABI v5 addition).  No host sync.
 *
 * usv_sde_squash_forward(s, epoch, mean, lat, row stride, std, act [n][A], act_env [n][A], logp [n],
 * gauss [n][A] or NULL, var [n][A] or NULL), one launch:
 *   gauss_k = mean_k + noise_k                            <- sample: mean + get_noise (bit-equal to
 *                                                            usv_sde_sample's act)
 *   act_k   = tanh(gauss_k)                               <- TanhBijector.forward (actions_from_params)
 *   om_k    = 4 t / (1 + t)^2, t = exp(-2 |gauss_k|)      <- 1 - tanh^2 of TanhBijector.log_prob_correction,
 *                                                            without its subtraction
 *   act_env_k = low_k + ((act_k + 1) * 0.5) * (high_k - low_k)   <- policy.unscale_action
 *   logp    = sum_k (-(gauss_k - mean_k)^2 / (2 s2_k) - 0.5 ln s2_k - 0.5 ln 2 pi - ln(om_k + 1e-6))
 *                                                         <- log_prob: the Gaussian term at gauss itself (SB3
 *                                                            takes it at atanh(clamp(act))) minus the correction
 *   var_k                                                 <- proba_distribution: mm(latent_sde ** 2, std ** 2)
 * gauss and var are what the backward needs of the forward; NULL together on a call that is not differentiated.
 *
 * usv_sde_squash_backward(s, epoch, mean, lat, row stride, std, gauss, var, g_act [n][A] or NULL, g_logp [n] or
 * NULL (NULL: zeros), g_mean [n][A], g_lat rows of latent_dim floats, its row stride, g_std [latent_dim][A],
 * scratch), two launches on the stream, replaces autograd through sample_weights' rsample, get_noise's bmm,
 * proba_distribution's mm and log_prob: the gradients of sum(g_act act) + sum(g_logp logp) with respect to
 * mean, lat (through the noise and the variance: learn_features) and std (through the matrix std z and the
 * variance), with the normals rebuilt from (seed, gid, epoch, element) as the forward built them.  Floats past
 * latent_dim in a strided g_lat row are not written.  g_std's sum over rows has no atomics and a fixed order
 * (csrc/usv_sde_math.hpp): partials of ceil(n / 1024) rows each in scratch, which holds
 * usv_sde_squash_scratch_floats(s) = P * latent_dim * act_dim floats (0 for a usv_sde that would be refused),
 * then one sum per element.  Two backward calls that share a scratch must be stream-ordered.
 *
 * USV_ERR_ARG, before any HIP call, for everything usv_sde_sample refuses, and: exactly one of gauss / var
 * NULL (forward); a NULL gauss, var or scratch, a g_lat or scratch that is not 16-B aligned, a g_lat row
 * stride below latent_dim or not a multiple of 4 (backward).  Then the device-memory checks. */
int usv_sde_squash_forward(const usv_sde* s, uint32_t epoch, const float* mean_dev, const float* lat_dev,
                           size_t lat_row_stride_floats, const float* std_dev, float* act_dev, float* act_env_dev,
                           float* logp_dev, float* gauss_dev, float* var_dev, void* stream);
size_t usv_sde_squash_scratch_floats(const usv_sde* s);
int usv_sde_squash_backward(const usv_sde* s, uint32_t epoch, const float* mean_dev, const float* lat_dev,
                            size_t lat_row_stride_floats, const float* std_dev, const float* gauss_dev,
                            const float* var_dev, const float* g_act_dev, const float* g_logp_dev, float* g_mean_dev,
                            float* g_lat_dev, size_t g_lat_row_stride_floats, float* g_std_dev, float* scratch_dev,
                            void* stream);

/* PPO's update-time head: SB3's ActorCriticPolicy.evaluate_actions for StateDependentNoiseDistribution (the
 * log-probability of stored actions under the current policy, no noise) with PPO's clipped surrogate on the same
 * row, and its backward.  Additive (ABI v5 addition); handle-free, stream-ordered, no host sync.  Of the usv_sde
 * only latent_dim, act_dim and reserved (= 0) are read: no noise is drawn, so n, seed, gid0, the bounds and the
 * epoch do not enter, and the row count is the call's `rows` (PPO's last minibatch may be short).
 *
 * usv_sde_eval_forward(s, rows, mean [rows][A], lat rows of latent_dim floats, row stride, std [latent_dim][A],
 * act [rows][A], old_logp [rows] or NULL, adv [rows] or NULL, clip, logp [rows], sur [rows] or NULL, ratio [rows]
 * or NULL, var [rows][A] or NULL), one launch:
 *   var_k   = sum_j (lat_j lat_j) (std_jk std_jk)         <- proba_distribution: usv_sde_sample's var_k bit for bit
 *   logp    = sum_k (-(act_k - mean_k)^2 / (2 s2_k) - 0.5 ln s2_k - 0.5 ln 2 pi),  s2_k = var_k + 1e-6
 *                                                         <- log_prob: bit-equal to usv_sde_sample's logp for its act
 * and, with old_logp, adv, sur and ratio (all four or none),
 *   ratio   = exp(logp - old_logp)                        <- PPO.train: th.exp(log_prob - rollout_data.old_log_prob)
 *   sur     = min(ratio adv, clamp(ratio, 1 - clip, 1 + clip) adv)    <- policy_loss_1, policy_loss_2, th.min
 * var is what the backward needs of the forward beyond its outputs; NULL on a call that is not differentiated.
 *
 * usv_sde_eval_backward(s, rows, mean, lat, row stride, std, act, var, ratio or NULL, adv or NULL, clip, g_logp
 * [rows] or NULL, g_sur [rows] or NULL (NULL: zeros), g_mean [rows][A], g_lat rows of latent_dim floats or NULL, its
 * row stride, g_std [latent_dim][A], scratch), two launches on the stream: the gradients of sum(g_logp logp) +
 * sum(g_sur sur) with respect to mean, lat (through the variance; NULL where the latent is detached, PPO's default,
 * and then nothing of [rows][latent_dim] is written) and std, as torch autograd gives them for Normal.log_prob, exp,
 * clamp and min, ties included (csrc/usv_sde_math.hpp).  act, old_logp and adv are data: no gradient.  g_std's sum
 * over rows is usv_sde_squash_backward's: no atomics, a fixed order, partials in scratch of
 * usv_sde_eval_scratch_floats(s, rows) = P * latent_dim * act_dim floats (0 for arguments that would be refused).
 * Two backward calls that share a scratch must be stream-ordered.
 *
 * USV_ERR_ARG, before any HIP call, for a NULL usv_sde, act_dim not 1 or 2, latent_dim outside [4, 4096] or not a
 * multiple of 4, reserved != 0, rows <= 0, a row stride below latent_dim or not a multiple of 4 (lat; g_lat where
 * set), only some of old_logp / adv / sur / ratio (forward) or of ratio / adv (backward), g_sur without ratio, a
 * negative or NaN clip where the surrogate is asked for, a NULL scratch or other needed buffer, a lat, g_lat or
 * scratch that is not 16-B aligned or another buffer that is not 4-B aligned.  Then the device-memory checks. */
int usv_sde_eval_forward(const usv_sde* s, int32_t rows, const float* mean_dev, const float* lat_dev,
                         size_t lat_row_stride_floats, const float* std_dev, const float* act_dev,
                         const float* old_logp_dev, const float* adv_dev, float clip, float* logp_dev, float* sur_dev,
                         float* ratio_dev, float* var_dev, void* stream);
size_t usv_sde_eval_scratch_floats(const usv_sde* s, int32_t rows);
int usv_sde_eval_backward(const usv_sde* s, int32_t rows, const float* mean_dev, const float* lat_dev,
                          size_t lat_row_stride_floats, const float* std_dev, const float* act_dev, const float* var_dev,
                          const float* ratio_dev, const float* adv_dev, float clip, const float* g_logp_dev,
                          const float* g_sur_dev, float* g_mean_dev, float* g_lat_dev, size_t g_lat_row_stride_floats,
                          float* g_std_dev, float* scratch_dev, void* stream);

/* Device replay buffer: SB3's ReplayBuffer (common/buffers.py: add, sample, _get_samples with
 * optimize_memory_usage=False and handle_timeout_termination=True) and the terminal-observation
 * substitution of OffPolicyAlgorithm._store_transition, for windows of k frames of d floats that evolve by
 * the VecFrameStack rule (usv_wrap_step).  It keeps one frame of obs and one of next_obs per transition
 * where SB3 keeps two k d stacks.  Handle-free and stream-ordered like usv_rollout_*; additive (ABI v5
 * addition).  No host sync: the ring position is the caller's (SB3's pos / full), passed as the 64-bit
 * step number c = 0, 1, .. of the call (counted since the buffers were new or the caller started over)
 * and, to the gather, as count = the number of completed transitions.  tests/replay_ref.py restates the
 * full-storage buffer; every gathered output equals it bit for bit.
 *
 * The ring has rows = R transitions per env (SB3: buffer_size // n_envs); transition c lives in slot
 * c % R.  frames is [n][R + k - 1][d], env-major: the frame of step c is row c mod (R + k - 1), the k - 1
 * older frames of the first window are rows R .. R + k - 2.  next_frame is [R][n][d], act [R][n][act_dim],
 * rew [R][n] float32, done / timeout / age [R][n] uint8, age_now [n] uint8 (the caller sets it to k - 1
 * before step 0).  csrc/usv_replay_math.hpp holds the arithmetic.
 *
 * usv_replay_put_obs(rp, c, stacked, row stride, act), before env step c      <- add: observations, actions
 *   stores the newest d columns of each stacked row [k d] (any 4-B-aligned base, row stride >= k d floats:
 *   DeviceWrappers.stacked is read in place) as the frame of step c (at c == 0 the whole window: the
 *   older columns go to the prologue rows as they are, cleared slots included), act[slot] = act_dev
 *   [n][act_dim] and age[slot] = age_now.
 * usv_replay_put_step(rp, c, rew, reward_bytes, term, trunc, next_stacked, row stride, final_stack), after
 * env step c:                                                  <- add: rewards, dones, timeouts, next_obs
 *   rew[slot] = float32(reward); done[slot] = term | trunc; timeout[slot] = trunc & !term (the adapter's
 *   TimeLimit.truncated); next_frame[slot] = the newest d columns of final_stack [n][k d] (usv_wrap_step's)
 *   for a done env (_store_transition: next_obs = terminal_observation) and of next_stacked, the window
 *   after the step, otherwise (only those rows of either are read); age_now = 0 for a done env, else
 *   min(age_now + 1, k - 1).
 * usv_replay_gather(rp, count, idx_dev [B] int64, B, out...): for i = idx[b] = slot * n + e with slot in
 * [0, min(count, R)), one launch writes                                       <- _get_samples
 *   obs_out[b] [k d]: the stacked window of that transition; next_obs_out[b] [k d]: its next_obs;
 *   act_out[b] [act_dim]; done_out[b] = float32(done) * (1 - float32(timeout)); rew_out[b].
 *   Slot j of obs (0 = oldest) is live when j >= k - 1 - age, slot j of next_obs when slot j + 1 of obs is
 *   (its newest always); a cleared element is +0.0, or x * 0.0f with USV_REPLAY_CLEAR_KEEPS_SIGN.
 *   An idx outside [0, min(count, R) * n) is not dereferenced: its outputs are NaN and *bad_count is
 *   incremented (never reset by the library); the call still returns USV_OK.
 * Preconditions the library cannot check: the calls of a run pass c = 0, 1, .. with put_obs(c) before
 * put_step(c); the windows evolve by the VecFrameStack rule with exactly the dones given (a window reset
 * by hand between stores is not supported: start over at c = 0 with age_now = k - 1); and no gather runs
 * between put_obs(c) and put_step(c): the frame row just written is the one the oldest valid window
 * still needs.
 *
 * USV_ERR_ARG, before any HIP call, for a NULL usv_replay, n / rows / obs_width / act_dim <= 0, k outside
 * [1, 32], d < 1, k * d != obs_width, unknown flags or reserved != 0, a NULL buffer or one not aligned to
 * its element size, c < 0 or count < 0, a row stride below obs_width, reward_bytes not 4 / 8, B <= 0, a
 * NULL idx (or one not 8-B aligned) or output.  Then for a buffer that is not device memory of the device
 * that holds frames. */
#define USV_REPLAY_CLEAR_KEEPS_SIGN 1
typedef struct usv_replay {    /* caller-owned device buffers */
  int32_t n, rows, obs_width, act_dim;
  int32_t k, d;                /* n_stack and floats per frame; k * d == obs_width */
  int32_t flags;               /* USV_REPLAY_* */
  int32_t reserved;            /* 0 */
  float* frames;               /* [n][rows + k - 1][d] */
  float* next_frame;           /* [rows][n][d] */
  float* act;                  /* [rows][n][act_dim] */
  float* rew;                  /* [rows][n] */
  uint8_t* done;               /* [rows][n] */
  uint8_t* timeout;            /* [rows][n] */
  uint8_t* age;                /* [rows][n] */
  uint8_t* age_now;            /* [n] */
  int32_t* bad_count;          /* [1] indices the gather refused */
} usv_replay;
int usv_replay_put_obs(const usv_replay* rp, int64_t c, const float* stacked_dev, size_t row_stride_floats,
                       const float* act_dev, void* stream);
int usv_replay_put_step(const usv_replay* rp, int64_t c, const void* rew_dev, int32_t reward_bytes,
                        const uint8_t* term_dev, const uint8_t* trunc_dev, const float* next_stacked_dev,
                        size_t next_row_stride_floats, const float* final_stack_dev, void* stream);
int usv_replay_gather(const usv_replay* rp, int64_t count, const int64_t* idx_dev, int32_t B, float* obs_out,
                      float* act_out, float* next_obs_out, float* done_out, float* rew_out, void* stream);

/* N-step sampling: SB3 2.7's NStepReplayBuffer._get_samples on the same ring, one launch (ABI v5 addition;
 * usv_replay and what is stored do not change).  tests/replay_nstep_ref.py restates it.  For i = idx[b] =
 * slot * n + e and last = (count - 1) % R, the run walks s_j = (slot + j) % R, j = 0 .. n_steps - 1, and ends
 * at m: the first j with done[s_j], timeout[s_j] or s_j == last (a run crosses neither the write position
 * nor unwritten rows), else n_steps - 1.
 *   obs_out[b], act_out[b]: those of (slot, e), as usv_replay_gather writes them;
 *   next_obs_out[b]: the next_obs of transition (s_m, e), rebuilt from the frame ring under that
 *   transition's own liveness; done_out[b] = float32(done) * (1 - float32(timeout)) of (s_m, e);
 *   rew_out[b] = rew[s_0] if m == 0 (the stored bits), else the float32 sum in the order j = 0 .. m of
 *   fl(rew[s_j] * g[j]), each product and each sum rounded to nearest on its own (no fused multiply-add);
 *   discount_out[b] = g[m + 1], the factor of the target Q.
 * discount_table_host is g[0 .. n_steps] in host memory, read during the call and passed to the kernel by
 * value: the caller's float32(gamma ** j), the power taken in double (g[0] = 1).
 * Two documented differences from SB3: it computes gamma ** float32 in float32 (within 1 ulp of such a
 * table), and it adds the terms behind m as +0.0 (visible only for a return of -0.0).
 * A bad idx gives NaN in all six outputs and counts in *bad_count.  The preconditions are those of
 * usv_replay_gather.  USV_ERR_ARG, before any HIP call, for everything usv_replay_gather refuses, n_steps
 * outside [1, 32], a NULL table or a table entry that is not finite. */
int usv_replay_gather_nstep(const usv_replay* rp, int64_t count, const int64_t* idx_dev, int32_t B, int32_t n_steps,
                            const float* discount_table_host /* [n_steps + 1] */, float* obs_out, float* act_out,
                            float* next_obs_out, float* done_out, float* rew_out, float* discount_out, void* stream);

/* ---- Fused SAC update: SB3's SAC.train lines for the TD target, the twin-critic loss, the actor and
 * entropy-coefficient losses (sac/sac.py; TD3's target without the entropy term) and common/utils.py's
 * polyak_update (ABI v5 additions).  Handle-free and stream-ordered like the usv_sde_* entries: the caller supplies
 * every buffer, f32 on one device and 4-B aligned; USV_ERR_ARG with a usv_last_error message, before any launch, for
 * what is refused.  The arithmetic and the fixed summation order are gym-usv_amd/csrc/usv_sac_math.hpp's;
 * tests/sac_loss_ref.py restates them.  All scalars that training changes (ent, log_ent, the upstream gradients) are
 * device scalars: no entry reads the device.
 *
 * scratch: usv_sac_scratch_floats(rows) floats (0 for rows < 1), 16-B aligned, zeroed once when it is allocated;
 * a call leaves its first word zero again.  Calls that share a scratch must be stream-ordered.  The losses do not
 * depend on the grid, the stream or the order in which blocks end: they are bitwise reproducible.
 *
 * usv_sac_critic_loss, rows [rows] each:
 *   qn = min(q1_next, q2_next) (a NaN stays);  with ent and logp_next  qn -= ent[0] * logp_next
 *   target = rewards + ((1 - dones) * disc) * qn      disc = discounts[i], or gamma where discounts is NULL
 *   loss[0] = 0.5 * (mean((q1 - target)^2) + mean((q2 - target)^2))
 *   g_q1 = (q1 - target) / rows, g_q2 likewise: the gradients at unit upstream (both optional: NULL under no_grad)
 * ent and logp_next come together (both NULL: TD3's target).
 *
 * usv_sac_policy_loss:
 *   actor_loss[0] = mean(ent[0] * logp - min(q1_pi, q2_pi))
 *   ent_loss[0]   = -mean(log_ent[0] * (logp + target_entropy))       only with log_ent (then ent_loss is required)
 *   g_logp = ent / rows;  g_q1 = -w / rows, g_q2 = -(1 - w) / rows, w = 1, 0.5, 0 for q1_pi <, ==, > q2_pi
 *   g_log_ent[0] = -mean(logp + target_entropy)
 * ent is data; every g_* is optional.
 *
 * usv_sac_loss_backward: o_k[i] = g_k[i] * up[0] for the up-to-three row gradients whose o_k is given (o1 is
 * required), and os[0] = gs[0] * up_s[0] where os is given.  A NULL up (up_s) writes zeros: the loss took no part
 * in what was differentiated.
 *
 * usv_polyak_update: dst = (dst * float(1 - tau)) + (float(tau) * src) over n_pairs tensor pairs in one launch, 1 - tau
 * taken in double.  pairs_host is read during the call.  table_dev: usv_polyak_table_bytes' worth of device memory,
 * 8-B aligned, that the call fills (after a device synchronise, and synchronising again) when upload != 0 and only
 * reads otherwise: upload whenever pairs_host has changed.  Pairs with numel == 0 are skipped (their pointers are not
 * looked at); a call with nothing left launches nothing.  Refused: n_pairs < 1, a NULL pointer, numel < 0, a pointer
 * that is not 4-B aligned, src == dst, tau outside [0, 1], a table that is too small. */
typedef struct usv_polyak_pair {
  const float* src;            /* the parameters */
  float* dst;                  /* the target's, updated in place */
  int64_t numel;
} usv_polyak_pair;
size_t usv_sac_scratch_floats(int32_t rows);
int usv_sac_critic_loss(int32_t rows, const float* q1, const float* q2, const float* q1_next, const float* q2_next,
                        const float* rewards, const float* dones, const float* ent, const float* logp_next,
                        const float* discounts, float gamma, float* target, float* loss, float* g_q1, float* g_q2,
                        float* scratch, void* stream);
int usv_sac_policy_loss(int32_t rows, const float* logp, const float* q1_pi, const float* q2_pi, const float* ent,
                        const float* log_ent, float target_entropy, float* actor_loss, float* ent_loss, float* g_logp,
                        float* g_q1, float* g_q2, float* g_log_ent, float* scratch, void* stream);
int usv_sac_loss_backward(int32_t rows, const float* up, const float* g1, const float* g2, const float* g3, float* o1,
                          float* o2, float* o3, const float* up_s, const float* gs, float* os, void* stream);
size_t usv_polyak_table_bytes(const usv_polyak_pair* pairs_host, int32_t n_pairs);
int usv_polyak_update(const usv_polyak_pair* pairs_host, int32_t n_pairs, void* table_dev, size_t table_bytes,
                      int32_t upload, double tau, void* stream);

/* ---- CAPS regulariser: Conditioning for Action Policy Smoothness (Mysore et al., ICRA 2021), the lambda_t, lambda_s
 * and eps_s keys of the reference's config_sac (train_test/config.py:34-36), which only the CAPS fork of SB3 takes
 * (ABI v5 additions).  Handle-free and stream-ordered like the usv_sac_* entries, with their rules for buffers (f32
 * on one device, 4-B aligned), for the scratch and for what is refused.  The arithmetic, the counter layout and the
 * summation order are gym-usv_amd/csrc/usv_caps_math.hpp's; tests/caps_ref.py restates them.
 *
 * usv_caps_perturb, obs and out [rows, width], contiguous:
 *   out[r, j] = obs[r, j] + (eps * z)     z: normal j % 4 of Philox4x32-10 block j / 4 with key seed and counter
 *                                         (r lo, r hi, epoch, j / 4), Box-Muller as the usv_sde_* entries take it
 * A row's noise depends on r, seed and epoch alone.  out may be obs itself; any other overlap is undefined.
 *
 * usv_caps_loss, mean, mean_next and mean_near [rows, act_dim] (the actor's pre-squash means at the observations,
 * the next observations and the perturbed ones), pi = tanh(mean) where squash != 0 and mean otherwise:
 *   out3[1] = temporal = mean_i ||pi(mean_i) - pi(mean_next_i)||_2
 *   out3[2] = spatial  = mean_i ||pi(mean_i) - pi(mean_near_i)||_2
 *   out3[0] = loss     = lambda_t * temporal + lambda_s * spatial
 *   g_mean, g_next, g_near [rows, act_dim]: the gradients of loss at unit upstream (each optional: NULL under
 *   no_grad); a row at zero distance contributes zero (the subgradient torch takes), a NaN stays NaN.
 * The backward is usv_sac_loss_backward with rows * act_dim for rows and these three arrays.
 * scratch: usv_sac_scratch_floats(rows) floats, as the usv_sac_* entries use it.
 * Refused: rows < 1, width < 1, act_dim outside [1, 8], rows * width or rows * act_dim above 2^31 - 1, an eps,
 * lambda_t or lambda_s that is NaN, infinite or negative, and what the usv_sac_* entries refuse of buffers. */
int usv_caps_perturb(int32_t rows, int32_t width, const float* obs, float* out, float eps, uint64_t seed,
                     uint32_t epoch, void* stream);
int usv_caps_loss(int32_t rows, int32_t act_dim, int32_t squash, const float* mean, const float* mean_next,
                  const float* mean_near, float lambda_t, float lambda_s, float* out3 /* loss, temporal, spatial */,
                  float* g_mean, float* g_next, float* g_near /* each [rows, act_dim] or NULL */,
                  float* scratch /* usv_sac_scratch_floats(rows) */, void* stream);

/* ---- Fused optimizer step: torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam.step() (torch 2.x,
 * amsgrad=False, weight_decay=0, maximize=False, the non-capturable path) over a whole list of tensors: one launch
 * without clipping, two with it, per 96 tensors of the list (ABI v5 additions).  Handle-free and stream-ordered like
 * the usv_sac_* entries.  The arithmetic and the fixed summation order are gym-usv_amd/csrc/usv_optim_math.hpp's;
 * tests/optim_ref.py restates them.
 *
 * usv_adam_step, with t = step >= 1 the number of this step (the caller counts), scalars taken in double and cast
 * once to f32:
 *   bc1 = 1 - beta1^t;  step_size = lr / bc1;  bc2_sqrt = sqrt(1 - beta2^t)
 *   with max_grad_norm >= 0:  total = sqrt(sum g^2) over every element of every tensor, written to norm_out[0] (the
 *     norm before clipping, clip_grad_norm_'s return value);  coef = min(1, max_grad_norm / (total + 1e-6));
 *     g' = g * coef (always multiplied).  A NaN or inf gradient is not special-cased: an inf gives coef = 0 and NaN
 *     at that element, as in torch.  With max_grad_norm < 0: no clipping, g' = g, norm_out is not looked at.
 *   m = m + (g' - m) * (1 - beta1);  v = v * beta2 + ((1 - beta2) * g') * g'
 *   param = param - step_size * (m / (sqrt(v) / bc2_sqrt + eps))
 * grad is read and never written: the clipped gradient exists in registers only.  The sum is taken in a fixed order
 * that depends on the numels alone, so total and every updated value are bitwise reproducible.
 *
 * tensors_host is read during the call; tensors with numel == 0 are skipped (their pointers are not looked at).
 * m, v: the first and second moments, usv_adam_state_floats' worth of floats each, 16-B aligned, zero before step 1:
 *   the tensors' segments in list order, each padded to a multiple of 4 floats.
 * scratch: usv_adam_scratch_floats' worth of floats, 16-B aligned, zeroed once when it is allocated (a call leaves
 *   its first word zero again); needed with clipping only.  Calls that share a scratch must be stream-ordered.
 * Both size functions return 0 for a list usv_adam_step would refuse by n or numel.
 * Refused with USV_ERR_ARG before any launch: n < 1, NULL tensors, numel < 0, a NULL or not 4-B aligned param or
 * grad, param == grad, step < 1, an lr or eps that is NaN, infinite or negative, a beta outside [0, 1), a NaN
 * max_grad_norm, m, v or (with clipping) scratch that is NULL, not 16-B aligned or too small, clipping without
 * norm_out, a norm_out that is not 4-B aligned, above 2^31 - 1 chunks of 4096 elements, a buffer that is no device
 * pointer on the device that holds m. */
typedef struct usv_adam_tensor {
  float* param;                /* updated in place */
  const float* grad;
  int64_t numel;
} usv_adam_tensor;
size_t usv_adam_state_floats(const usv_adam_tensor* tensors_host, int32_t n);
size_t usv_adam_scratch_floats(const usv_adam_tensor* tensors_host, int32_t n);
int usv_adam_step(const usv_adam_tensor* tensors_host, int32_t n, float* m, float* v, size_t state_floats, int64_t step,
                  double lr, double beta1, double beta2, double eps, double max_grad_norm /* < 0: none */,
                  float* scratch, size_t scratch_floats, float* norm_out, void* stream);

/* ---- Fused PPO loss: the loss lines of SB3's PPO.train (ppo/ppo.py) for one minibatch, with approx_kl, clip_fraction
 * and common/utils.py's explained_variance (ABI v5 additions).  Handle-free and stream-ordered like the usv_sac_*
 * entries, with their rules for buffers (f32 on one device, 4-B aligned) and for what is refused.  The arithmetic
 * and the fixed summation order are gym-usv_amd/csrc/usv_ppo_math.hpp's; tests/ppo_loss_ref.py restates them.
 *
 * usv_ppo_loss, rows [rows] each; one call issues up to three launches:
 *   with normalize != 0 and rows > 1:  moments[0] = mean(adv);  moments[1] = std(adv), unbiased, two passes;
 *     a = (adv - mean) / (std + 1e-8);  otherwise a = adv and moments is not written
 *   ratio = exp(logp - old_logp);  policy_loss = -mean(min(ratio a, clamp(ratio, 1 - clip, 1 + clip) a))
 *   vp = values, or old_values + clamp(values - old_values, -clip_vf, clip_vf) where old_values is given
 *   value_loss = mean((returns - vp)^2);  entropy_loss = -mean(entropy), or -mean(-logp) where entropy is NULL
 *   out[0] = loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
 *   out[1..5] = policy_loss, value_loss, entropy_loss, approx_kl = mean((ratio - 1) - (logp - old_logp)),
 *               clip_fraction = mean(|ratio - 1| > clip)
 *   g_logp, g_values, g_entropy [rows]: the gradients of loss at unit upstream (each optional: NULL under no_grad;
 *   g_entropy needs entropy); torch.min's and torch.clamp's ties as autograd has them.  The backward is
 *   usv_sac_loss_backward on the three arrays.
 * adv, old_logp, old_values and returns are data.  Without old_values, clip_vf is 0.
 *
 * usv_ppo_explained_variance: out[0] = 1 - var(returns - values) / var(returns), population variances in the same
 * two-pass form, NaN where var(returns) == 0; two launches.
 *
 * scratch: usv_ppo_scratch_floats(rows) floats (0 for rows < 1), 16-B aligned, zeroed once when it is allocated; a
 * call leaves its first word zero again.  Calls that share a scratch must be stream-ordered.  Nothing depends on the
 * grid, the stream or the order in which blocks end: every output is bitwise reproducible.
 * Refused: rows < 1, a clip or clip_vf that is NaN, infinite or negative, a clip_vf other than 0 without old_values,
 * g_entropy without entropy, and what the usv_sac_* entries refuse of buffers. */
size_t usv_ppo_scratch_floats(int32_t rows);
int usv_ppo_loss(int32_t rows, const float* logp, const float* old_logp, const float* adv, const float* values,
                 const float* old_values /* NULL: no clip_range_vf */, const float* returns,
                 const float* entropy /* NULL: -logp */, int32_t normalize, float clip, float clip_vf, float ent_coef,
                 float vf_coef, float* moments /* 2 floats */, float* out /* loss + 5 statistics */, float* g_logp,
                 float* g_values, float* g_entropy /* each [rows] or NULL */, float* scratch, void* stream);
int usv_ppo_explained_variance(int32_t rows, const float* values, const float* returns, float* out /* 1 float */,
                               float* scratch, void* stream);

/* ---- Graph-capturable update: the step and noise counters of the entries above in device memory (ABI v5
 * additions).  A captured HIP graph freezes kernel arguments, so a replay of usv_adam_step would repeat the bias
 * correction of the captured step and a replay of a noise entry would redraw the captured epoch's noise.  These forms
 * read the counters from device words that kernels inside the graph advance.  Handle-free and stream-ordered; every
 * existing entry, its kernel and its results are unchanged.  No entry here allocates, synchronises or copies from the
 * host: all are legal while `stream` is capturing, and the device-memory checks of the buffers stay on (the runtime
 * answers hipPointerGetAttributes during a capture).
 *
 * usv_counter_add: word_dev[0] += inc, wrapping at 2^32 as a host uint32 epoch does; one launch of one thread.
 *
 * usv_sde_sample_dev / usv_sde_weights_dev / usv_sde_squash_forward_dev / usv_sde_squash_backward_dev /
 * usv_caps_perturb_dev: the entry without _dev, with the epoch read from epoch_dev[0] by the kernel (once per wave)
 * where the other takes `epoch` as an argument.  Same kernel body, bit-equal results for an equal epoch.  A backward
 * reads the word when it runs: the word must not change between a forward and its backward.
 *
 * usv_adam_step_dev: usv_adam_step with the step number and lr in the clock block clock_dev (usv_adam_clock_bytes()
 * bytes of device memory, 16-B aligned; clock_bytes is its size):
 *     offset 0   double  lr                   the caller writes it (stream-ordered) and may change it between steps
 *     offset 8   int64   step                 the number of the last step taken: 0 before the first
 *     offset 16  float   step_size, bc2_sqrt  of that step, derived on the device
 * One launch of one thread, ahead of the call's other launches, sets step += 1 and derives step_size = lr / (1 -
 * beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) in double, each cast once to f32 (adam_clock_scalars,
 * gym-usv_amd/csrc/usv_optim_math.hpp): once per call however many launches the list takes, so one launch more than
 * usv_adam_step.  The device's pow is not the host's: the two scalars are within 1 f32 ulp of usv_adam_step's, and where
 * they are equal so is every result.  The betas, eps and max_grad_norm stay arguments.
 *
 * usv_polyak_prepare: usv_polyak_update's table upload alone (it synchronises; nothing is launched).  While `stream` is
 * capturing, usv_polyak_update with upload != 0 is refused with USV_ERR_ARG before it synchronises: prepare first.
 *
 * Refused with USV_ERR_ARG before any HIP call: a NULL or not 4-B aligned word_dev or epoch_dev, a NULL or not 16-B
 * aligned clock_dev, clock_bytes below usv_adam_clock_bytes(), and what the entry without _dev refuses. */
int usv_counter_add(uint32_t* word_dev, uint32_t inc, void* stream);
int usv_sde_sample_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat, size_t stride,
                       const float* std, float* act, float* act_env, float* logp, void* stream);
int usv_sde_weights_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* std, float* w, void* stream);
int usv_sde_squash_forward_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat,
                               size_t stride, const float* std, float* act, float* act_env, float* logp, float* gauss,
                               float* var, void* stream);
int usv_sde_squash_backward_dev(const usv_sde* s, const uint32_t* epoch_dev, const float* mean, const float* lat,
                                size_t stride, const float* std, const float* gauss, const float* var,
                                const float* g_act, const float* g_logp, float* g_mean, float* g_lat, size_t g_stride,
                                float* g_std, float* scratch, void* stream);
int usv_caps_perturb_dev(int32_t rows, int32_t width, const float* obs, float* out, float eps, uint64_t seed,
                         const uint32_t* epoch_dev, void* stream);
size_t usv_adam_clock_bytes(void);
int usv_adam_step_dev(const usv_adam_tensor* tensors_host, int32_t n, float* m, float* v, size_t state_floats,
                      void* clock_dev, size_t clock_bytes, double beta1, double beta2, double eps,
                      double max_grad_norm /* < 0: none */, float* scratch, size_t scratch_floats, float* norm_out,
                      void* stream);
int usv_polyak_prepare(const usv_polyak_pair* pairs_host, int32_t n_pairs, void* table_dev, size_t table_bytes);

/* Select the step-kernel variant of a usv-simple / usv-asmc-simple handle (verification and
 * tuning: every variant computes bit-identical outputs, tests/test_gpu_*.py compare them bitwise).
 * No reference counterpart; usv_create picks the tuned default.
 *   kind 1: fused wave kernel (epb 16 | 32 | 64 envs per 256-thread block)
 *   kind 2: split dynamics + wave scan (epb 8 | 16 | 32; f64 usv-simple window also 64)
 *   kind 3: one launch, wave 0 of each 4-wave block runs the block's dynamics, then the wave scan
 *           (f64 usv-simple, window lidar; epb 32 | 64)
 *   kind 4 / 5: split / fused block-queue step (epb 128; kind 5 also 16), f32 window lidar, cap <= 32
 *   kind 6: usv-asmc-simple only: the ASMC chain in its own launch, then the fused block-queue step
 *           (epb 128 | 16), f32 window lidar, cap <= 32
 *   lid: lidar variant bits (0 brute, 3 brute + blind-sector skip + unroll, 7 angular window); kinds 4-6
 *        also take 0x100 / 0x200: obs rows stored as 32-B-aligned env-pair spans forced on / off (default:
 *        on from 196 608 envs, where the rows go to DRAM)
 * Waits for in-flight launches first.  USV_ERR_ARG if the handle's config cannot run it. */
int usv_set_kernel_variant(void* handle, int32_t kind, int32_t epb, int32_t lid);

/* UsvSimpleEnv.ignore_obstacles (gym_usv/envs/simple_env.py:49; UsvSimpleASMCEnv inherits it), an
 * attribute the reference's users set after make().  While it is on, for usv-simple / usv-asmc-simple:
 *   - every lidar reading is the maximum range (:222-224): obs[15:143] = 100 / 100 = 1.0f exactly;
 *   - the reward has no -20 collision term (:155): rew_dev is the sum of the other terms;
 *   - no env terminates on an obstacle (:334): term_dev is 0, done_dev equals trunc_dev;
 *   - kinematics, the ASMC chain, closest point, obs header, truncation, TimeLimit and the info rows are
 *     those of the scanning step, bit for bit (the same device code);
 *   - resets draw as always, obstacles included (the reference draws them, and a later toggle-off finds
 *     them); a reset obs carries the stale sensor_data (:302, :47), which follows the mode of the last
 *     step taken: 1.0 after an ignoring step, the last real scan after a scanning one, zeros for a
 *     never-stepped env.
 * usv_step / usv_step_ex then launch a scan-free kernel instead of the installed step variant, which is
 * kept and used again after toggle-off.  Such a step leaves USV_FIELD_SCAN_VALID = 2: "the stale scan is
 * 128 readings of 100"; a reset turns that into USV_FIELD_SENSOR_LAST = 100 and scan_valid = 0.
 * The setter waits for in-flight launches first; USV_ERR_ARG for the legacy *-v0 ids.  The getter
 * returns 0 / 1, or a negative usv_status.  USV_FLAG_IGNORE_OBSTACLES sets the initial value. */
int usv_set_ignore_obstacles(void* handle, int32_t on);
int usv_get_ignore_obstacles(void* handle);

/* Field metadata: values per env, 1 if int32, name. */
int usv_field_info(void* handle, int32_t field, int32_t* per_env, int32_t* is_int,
                   const char** name);
/* Synchronous host copies (device synchronised first). `bytes` must equal
 * num_envs * per_env * (is_int ? 4 : 8). */
int usv_get_field(void* handle, int32_t field, void* host, size_t bytes);
int usv_set_field(void* handle, int32_t field, const void* host, size_t bytes);

/* Whole-state blob (all fields in enum order, host layout as above): env checkpoint. */
size_t usv_state_bytes(void* handle);
int usv_get_state(void* handle, void* host, size_t bytes);
int usv_set_state(void* handle, const void* host, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* USV_HIP_H */
