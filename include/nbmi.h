/*
 * nbmi.h - C ABI of the MI355X-native N-body backend (libnbmi.so).
 *
 * This is the drop-in boundary for the reference's N-body *backend protocol*: the duck-typed
 * object returned by create_gpu_simulation() (reference nbody/gpu_backend.py:623-679) whose
 * methods are step / compute_colors / get_positions / get_velocities / get_colors / sync
 * (reference class CUDASimulation, nbody/gpu_backend.py:336-409; Metal twin
 * nbody/metal/metal_backend.py:246, 487-599).  One entry point per protocol method, plain
 * pointers and sizes only.  All functions return 0 on success and a negative code on failure;
 * nbmi_last_error() gives the message (thread-local).  A handle is used from one host thread
 * at a time and owns one HIP stream.
 *
 * Body arrays crossing the boundary are the reference's layouts: positions / velocities are
 * C-order (N,3), masses (N,), float64 in (as the reference constructors take them,
 * gpu_backend.py:339-356), float32 positions / colours and float64 velocities out
 * (gpu_backend.py:394-404).  Rows are always in the caller's original body order.
 */
#ifndef NBMI_H
#define NBMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct nbmi_sim nbmi_sim;

#define NBMI_METHOD_BARNES_HUT 0 /* octree build + tree walk: nbody/simulation.py:63-305        */
#define NBMI_METHOD_DIRECT 1     /* all-pairs O(N^2): nbody/gpu_backend.py:145-257               */

#define NBMI_OK 0
#define NBMI_ERR_ARG (-1)
#define NBMI_ERR_HIP (-2)
#define NBMI_ERR_NODEV (-3)
#define NBMI_ERR_CAPACITY (-4) /* octree needs more node rows than allocated (4N, at most 178 M) */

/* Number of visible HIP devices (0 if none / no driver).  Replaces the probe in
 * detect_backend()/_check_cuda(), nbody/gpu_backend.py:36-70. */
int nbmi_device_count(void);

/* Message of the last failing call on this thread ("" if none). */
const char *nbmi_last_error(void);

/* Constructor: CUDASimulation.__init__ (gpu_backend.py:339-366) /
 * MetalBarnesHutSimulation.__init__(…, theta) (metal_backend.py:252-254).  Copies the three
 * host arrays to the device; the caller keeps ownership.  Returns NULL on failure. */
nbmi_sim *nbmi_create(int64_t n, const double *positions_xyz, const double *velocities_xyz,
                      const double *masses, double G, double softening, double damping,
                      double theta, int method, int device);

/* Constructor with DEVICE-SIDE initial conditions: the bodies are drawn on the
 * GPU from generate_distribution's formulas (tools/presets.py:104-232 "galaxy" / "collision",
 * :234-295 "spiral", :350-397 "cluster": unit masses; :609-684 "filament", the cosmic web: masses
 * 0.1) with a counter-based Philox4x32-10 stream keyed by `seed`, so a 10-50 M-body start needs no
 * host generator and no multi-GB upload.  Statistical parity with the NumPy generator (another
 * random stream), and per-body parity, to the bound recorded in DESIGN.md, with the host replay of
 * the same stream in tests/icgen_ref.py; the same (seed, n, radius, G) always gives the same
 * bodies.  G is used both for the rotation
 * curve / dispersions and for the simulation, as record() does (tools/record.py:747-758).  Body i
 * of the getters is the i-th generated body.  "filament" fails (NULL) in the ~1e-96 case that none
 * of its 512 grid nodes is active, as the reference does. */
#define NBMI_IC_GALAXY 0
#define NBMI_IC_COLLISION 1
#define NBMI_IC_CLUSTER 2
#define NBMI_IC_SPIRAL 3
#define NBMI_IC_FILAMENT 4
nbmi_sim *nbmi_create_generated(int distribution, int64_t n, double spawn_radius, uint64_t seed, double G,
                                double softening, double damping, double theta, int method, int device);
/* The generator's random function, computed on the host (known-answer tests). */
void nbmi_philox4x32_10(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
/* Masses (N,) float64 in the caller's order (state checkpoints of generated systems). */
int nbmi_get_masses_f64(nbmi_sim *sim, double *out);

void nbmi_destroy(nbmi_sim *sim);

/* step(dt): gpu_backend.py:368-386.  `substeps` consecutive steps of size dt are enqueued on
 * the handle's stream without host synchronisation (record() calls step() `substeps` times per
 * frame, tools/record.py:823-824).  Barnes-Hut: bounds -> keys -> sort -> octree -> walk with the
 * reference's kick-drift update fused in (simulation.py:308-317, 63-198, 201-278, 281-305). */
int nbmi_step(nbmi_sim *sim, double dt, int substeps);
/* Integrator of nbmi_step.
 *   NBMI_INTEGRATOR_KICK_DRIFT (default): the reference's v = (v + a dt) damping; x += v dt (simulation.py:291-305), a
 *     first-order scheme whose stored velocities lie half a step from the positions.
 *   NBMI_INTEGRATOR_LEAPFROG: synchronized kick-drift-kick, second order and time-reversible (damping 1).  With a the stored
 *     acceleration of the current positions, every substep is
 *       v <- v + a dt/2;  x <- x + v dt;  a <- F(x) (octree build + walk, or direct N^2);  v <- (v + a dt/2) damping
 *     and leaves (x, v) at the same instant with a = F(x).  Forces use the machinery of the current mode unchanged
 *     (octree and accepted sets, nbmi_set_force_precision, direct N^2).  The stored a is dropped on create, by
 *     nbmi_set_state, by a switch into leapfrog and when a capacity error is reported; the next nbmi_step then "primes"
 *     it with one extra force evaluation a = F(x) (inside the step, so force precision "auto" sees its dt).  The first
 *     leapfrog step allocates 24 bytes per body for a.  Getters, colours, frames and nbmi_diagnostics therefore see
 *     synchronized velocities (no half-step offset in K and E); nbmi_diagnostics and nbmi_get_accelerations_f64 leave the
 *     state and the stored a as they were.  A capacity error leaves the state at the last completed step, as in
 *     kick-drift.  Owner-mode handles and handles with a proper shard (nbmi_set_shard, in either order of the calls)
 *     refuse leapfrog with NBMI_ERR_ARG. */
#define NBMI_INTEGRATOR_KICK_DRIFT 0
#define NBMI_INTEGRATOR_LEAPFROG 1
int nbmi_set_integrator(nbmi_sim *sim, int integrator);
int nbmi_get_integrator(nbmi_sim *sim, int *out);
/* Multipole order of an applied Barnes-Hut cell term.
 *   NBMI_MULTIPOLE_MONOPOLE (default): a point mass at the cell's centre of mass - the reference's term; everything this
 *     header says elsewhere describes it.  A handle that never leaves it runs the force kernels and the octree build
 *     unchanged.  (The tree potential of nbmi_diagnostics / nbmi_get_potentials_f64 changed together with the mode, in
 *     both modes: see the note on near pairs there.)
 *   NBMI_MULTIPOLE_QUADRUPOLE: the octree, the opening test, the float64 re-decision of ties, the own-leaf rule and the
 *     node_mass > 0, dist_sq > eps^2 guards are untouched: a body's set of applied (body, node) terms at the handle's theta
 *     is the reference's, in both modes.  Only the VALUE of a term changes, and only for internal cells.  An internal
 *     cell n additionally carries the raw second moments of its bodies about its centre of mass c_n,
 *       P_ab = sum_j G m_j (x_j - c_n)_a (x_j - c_n)_b
 *     (six numbers, G folded in; raw, not traceless: the kernel is Plummer-softened, f(r) = -(r^2 + eps^2)^(-1/2), its
 *     Laplacian does not vanish, so the trace carries force).  A leaf has P = 0.  With d = c_n - x_i and
 *     u = |d|^2 + eps^2 (the dist_sq of the test) an applied cell term is
 *       a_i   += G M d u^(-3/2)                                                     (the monopole term, arithmetic unchanged)
 *              + [ 7.5 (d^T P d) u^(-7/2) - 1.5 tr(P) u^(-5/2) ] d  -  3 u^(-5/2) (P d)
 *       phi_i += - G M u^(-1/2)  +  1/2 [ tr(P) u^(-3/2) - 3 (d^T P d) u^(-5/2) ]
 *     the second-order Taylor term of sum_j G m_j f(x_i - x_j) about c_n (the dipole vanishes there); a = -grad phi holds
 *     term by term.  The correction is evaluated through e = d u^(-1/2) as u^(-2) [(7.5 e^T P e - 1.5 tr P) e - 3 P e], which
 *     forms nothing beyond u^(-2).
 *     Precision: the monopole part of a term is computed as the handle's force precision computes it (fp32, per-wave
 *     "auto", float64; the build's "auto" decision is unchanged).  The correction is fp32 arithmetic in every mode; in a
 *     float64 wave it starts from the float64 difference d rounded to fp32, not from the difference of fp32-rounded
 *     coordinates.  fp32 partial sums are emptied into float64 every 12 visits.
 *     nbmi_get_accelerations_f64, nbmi_step (kick-drift and leapfrog, damping included), nbmi_get_potentials_f64 and
 *     nbmi_diagnostics(with_potential = 1) all use the mode's terms, so E = K + W stays the energy of the force that moves
 *     the bodies.  In quadrupole mode nbmi_get_accelerations_f64 HONOURS force precision 1 (fp32) and 2 (float64); 0
 *     ("auto") has no wave flags without a step's dt and means fp32 (the monopole force pass is fp32 whatever the mode).
 *     `terms` of nbmi_diagnostics and the lane-accept count of nbmi_walk_counters after nbmi_get_accelerations_f64 are the
 *     same numbers in both modes; the other sixteen walk counters read 0 in quadrupole mode.  The mode's walk contains
 *     no instruction written by hand; two empty asm statements pin its scalar loads in place.
 *     One one-wave walk serves every size (no split walk below 280 k bodies, no XCD balance mode).  The first switch into
 *     the mode allocates 24 + 72 + 32 bytes per node row; every build of the mode also writes the rows the cell queries read
 *     and runs a bottom-up pass over the levels of the tree for the moments.
 *     Refused with NBMI_ERR_ARG: direct N^2 handles, owner-mode handles, handles with a proper shard (nbmi_set_shard, in
 *     either order of the calls: their exchanged rows carry no P).
 * A switch drops the stored leapfrog acceleration (the next step primes it in the new mode).  Environment NBMI_MULTIPOLE
 * ("quadrupole" or "1"; anything else means monopole) sets the initial value on handles that allow it. */
#define NBMI_MULTIPOLE_MONOPOLE 0
#define NBMI_MULTIPOLE_QUADRUPOLE 1
int nbmi_set_multipole(nbmi_sim *sim, int multipole);
int nbmi_get_multipole(nbmi_sim *sim, int *out);
/* Number of steps enqueued on this handle since it was created (every substep of nbmi_step counts).  The
 * recorder's Ctrl-C path asks the library, not its own bookkeeping, which frame the device has reached: an
 * interrupt is delivered when nbmi_step returns, before the caller can note that the step was taken
 * (tools/record.py:916-935 writes "state at the frame the device is at"). */
int64_t nbmi_step_count(nbmi_sim *sim);

/* compute_colors(max_speed): gpu_backend.py:388-392 (ramp of simulation.py:320-400). */
int nbmi_compute_colors(nbmi_sim *sim, double max_speed);

/* get_positions() -> (N,3) float32 (gpu_backend.py:394-396). */
int nbmi_get_positions_f32(nbmi_sim *sim, float *out_xyz);
/* get_velocities() -> (N,3) float64 (gpu_backend.py:398-400). */
int nbmi_get_velocities_f64(nbmi_sim *sim, double *out_xyz);
/* get_colors() -> (N,3) float32 (gpu_backend.py:402-404). */
int nbmi_get_colors_f32(nbmi_sim *sim, float *out_rgb);
/* sync(): gpu_backend.py:406-409.  Also reports deferred device-side errors.  NBMI_ERR_CAPACITY is
 * sticky on the device: from the substep whose octree did not fit, the bodies are no longer advanced
 * (they stay at the last completed step) until a sync / getter has reported the error once. */
int nbmi_sync(nbmi_sim *sim);

/* ---- supersets of the protocol (parity / measurement hooks) --------------------------- */

/* Full-precision state (float64 master copy kept on the device). */
int nbmi_get_positions_f64(nbmi_sim *sim, double *out_xyz);
/* Replace positions+velocities (resume from a state_%04d.npz, tools/record.py:728-733). */
int nbmi_set_state(nbmi_sim *sim, const double *positions_xyz, const double *velocities_xyz);

/* Build the octree for the CURRENT positions without advancing time (bounds, keys, sort,
 * node emission).  After it the tree queries below describe that tree. */
int nbmi_build_tree(nbmi_sim *sim);
/* Accelerations (N,3) float64 of the current positions (build + walk, no integration):
 * compute_forces_barnes_hut / compute_forces_*_cuda output. */
int nbmi_get_accelerations_f64(nbmi_sim *sim, double *out_xyz);
/* num_nodes as build_octree returns it (simulation.py:198), deepest level, root half-size
 * (compute_bounds, simulation.py:317) of the most recently built tree. */
int nbmi_tree_stats(nbmi_sim *sim, int64_t *num_nodes, int32_t *max_depth, double *bounds);
/* Octant-path keys of every body for the most recently built tree, original body order:
 * key_hi = levels 1..21 (3 bits per level, level 1 most significant, digit =
 * x>=cx | (y>=cy)<<1 | (z>=cz)<<2 as get_octant, simulation.py:38-49), key_lo = levels 22..42. */
int nbmi_get_keys(nbmi_sim *sim, uint64_t *key_hi, uint64_t *key_lo);
/* The keys the device actually sorts by, same layout: the octant digits relabelled along the 3-D Hilbert curve
 * (csrc/hilbert.h: the digit of a child depends on its octant and on the orientation of its cell; a bijection per
 * cell, so two bodies share exactly as many leading digits as with the octant digits, and nbmi_get_keys is the
 * decoded form of these).  Only the order of a cell's eight children differs from the octant order. */
int nbmi_get_sort_keys(nbmi_sim *sim, uint64_t *key_hi, uint64_t *key_lo);
/* Body indices in sort-key (octree DFS, children along the Hilbert curve) order for the most recently built tree:
 * order[r] = index, in the caller's numbering, of the r-th body along that order. */
int nbmi_get_order(nbmi_sim *sim, int32_t *order);
/* (level, path key) of every node of the most recently built tree (num_nodes entries,
 * unspecified order).  Keys of levels > 21 are reported as UINT64_MAX. */
int nbmi_get_cells(nbmi_sim *sim, int32_t *level, uint64_t *key, int64_t capacity);
/* Quadrupole mode, after nbmi_build_tree: nbmi_get_cells' (level, key) of every node plus its six second moments
 * {Pxx, Pyy, Pzz, Pxy, Pxz, Pyz} as the walk's fp32 records hold them, widened to float64 (num_nodes x 6; a leaf has no
 * record: zeros). */
int nbmi_get_cell_moments(nbmi_sim *sim, int32_t *level, uint64_t *key, double *moments6, int64_t capacity);
/* Per-phase device time in ms accumulated since the last reset:
 * [bounds+keys, sort, tree build, walk+integrate, other]; count = steps accumulated.
 * Enabling timers adds hipEvent records to every step. */
int nbmi_enable_timers(nbmi_sim *sim, int enable);
int nbmi_get_timers(nbmi_sim *sim, double *ms5, int64_t *count, int reset);
/* Work counters of the last counted walk (nbmi_get_accelerations_f64): [wave-level node visits,
 * lane-level visits, lane accepts, node-window misses for windows of 8/16/32/64 nodes,
 * non-sequential cursor moves, wave-level visits executed on each of the 8 XCDs, lane visits whose
 * opening test was a near-tie in fp32 and was re-decided in float64 like the reference
 * (simulation.py:252-258)] (17 values). */
int nbmi_walk_counters(nbmi_sim *sim, int64_t *out17);

/* ---- conservation diagnostics ---------------------------------------------------------------
 * Of the handle's current float64 state (positions x, velocities v as stored: the reference's kick-drift keeps them half
 * a step apart, so E = K + W carries an O(dt) oscillation), masses m, constant G, softening eps:
 *   M = sum m_i,  c = sum m_i x_i / M (0 when M == 0),  P = sum m_i v_i,  L = sum m_i (x_i X v_i) about the origin,
 *   K = 1/2 sum m_i |v_i|^2,  W = 1/2 sum m_i phi_i,  E = K + W.
 * phi_i is per unit mass of body i, G included:
 *   Barnes-Hut handle (tree potential): phi_i = - sum G M_n / sqrt(d^2 + eps^2) over exactly the terms the reference's
 *     walk applies to body i at the handle's theta (nbody/simulation.py:245-262): a node is accepted when it is a leaf or
 *     node_size / dist < theta, else opened; the body's own leaf is skipped; a term is applied only when node_mass > 0
 *     and dist_sq > eps^2, dist_sq = ((dx dx + dy dy) + dz dz) + eps^2 in float64.  G M_n and the centre of mass are the
 *     node's float64 moments (the double-double prefix sums of the build); a leaf uses its body's float64 position and
 *     G m.  A pair whose dist_sq rounds to eps^2 adds no force; it would add -G m / eps here, so the guard skips it too.
 *     The accepted sets are the force walk's: the same octree of the current positions, the same opening decision.
 *     Near pairs: the fp32 opening test carries an uncertainty band of at most 2^21 ulps of d^2, which covers its rounding
 *     only for pairs at least 3.3e-6 of the largest coordinate apart.  With softening 0, or one below that length, closer
 *     pairs exist; a cell closer than 8e-6 of the largest coordinate is then decided by the reference's float64 test
 *     outright, so `terms` and phi are the reference's there too.  (Before quadrupole mode was added such cells went by
 *     the fp32 test alone: on 2 048 bodies within 1e-3 of a point at coordinate 700, `terms` read 19 above the reference's
 *     1 628 049.)  Handles with a softening above 3.3e-6 of the largest coordinate are not affected.
 *   Direct handle (exact pair sum): phi_i = - sum_{j != i} G m_j / sqrt(|x_j - x_i|^2 + eps^2); with eps == 0 pairs at
 *     zero distance are skipped (as the force kernel skips them).
 * All arithmetic is float64 (sqrt and divide correctly rounded); the sums are per-block partials over the state rows
 * (the last step's key order; the caller's order before the first step, and always for direct handles) combined in a
 * fixed order without floating-point atomics: two calls on an unchanged state return the same bits, and the result does
 * not depend on the force precision or on whether the handle keeps float64 node records.
 * A call changes nothing that a later step reads (state and its order, the tree header, the "auto" precision flags, the
 * step count); the first call with the potential allocates 32 bytes per node row (Barnes-Hut) and 12 bytes per body.
 * Owner-mode handles (and handles with a shard set) are refused with NBMI_ERR_ARG, message "<call>: owner-mode handles are
 * not supported (...)".  n == 0 gives zeros (and terms = 0).  NBMI_ERR_CAPACITY from the call's own tree build is
 * reported with a step's message.
 *
 * out12 = {M, c[3], P[3], L[3], K, W}; W = NaN when with_potential == 0 (no tree is built, no walk runs).
 * *terms (may be NULL) = number of (body, node) terms applied to the potential (0 without it). */
int nbmi_diagnostics(nbmi_sim *sim, int with_potential, double *out12, int64_t *terms);
/* phi (N,) float64 in the caller's body order, as defined above. */
int nbmi_get_potentials_f64(nbmi_sim *sim, double *out);

/* ---- k-nearest-neighbour distances and densities -------------------------------------------
 * Of the handle's current float64 state, for every body i, exactly:
 *   d2(i, j)  = (dx dx + dy dy) + dz dz with dx = x_j - x_i, float64 in this association, no FMA.
 *   r2_k[i]   = the k-th smallest of the multiset {d2(i, j) : j != i}, counted with multiplicity.  Self is excluded by
 *               identity (equivalently: one zero entry is dropped); a coincident other body counts with d2 = 0.  The
 *               value does not depend on how ties are ordered and equals a brute force's bit for bit.
 *   mass_k[i] = m_i + sum of m_j over j != i with d2(i, j) <= r2_k[i].  Under ties this covers more than k bodies, which
 *               is what makes it independent of their order.  A sum of masses (not of G m): the query reads the masses,
 *               so handles with G == 0 work.  Summed in the order of the walk (fixed for a given state).
 *   rho[i]    = mass_k / (4.1887902047863905 (r2_k sqrt(r2_k))), the mean density inside the k-th neighbour sphere;
 *               +inf where r2_k == 0.
 * 1 <= k <= 64 and k <= N - 1, else NBMI_ERR_ARG with a message naming k and N.  Outputs are (N,) float64 in the caller's
 * body order; r2_k, mass_k and evals may each be NULL.  *evals = the number of (body, leaf) distances the call evaluated
 * (seeding, the search and the mass sum together): a measurement hook like nbmi_walk_counters, to judge the pruning.
 * Two calls on an unchanged state return the same bits.  A quadrupole or leapfrog handle returns a monopole kick-drift
 * handle's bits: the tree is the same.
 * A call changes nothing that a later step reads (state and its order, the tree header - saved and restored -, the
 * "auto" precision flags and force_all64 - the build runs without a dt -, the step count, the stored leapfrog
 * acceleration).  The first call allocates 16 bytes per body and - once for nbmi_knn, nbmi_fof and nbmi_pair_counts
 * together, by whichever is called first - 32 bytes per node row and 4 bytes per 64 bodies.  NBMI_ERR_CAPACITY from the
 * call's own tree build is reported with a step's message.
 * Refused with NBMI_ERR_ARG, message "<call>: ...": direct N^2 handles (there is no tree), owner-mode handles and
 * handles with a proper shard. */
int nbmi_knn(nbmi_sim *sim, int k, double *r2_k, double *mass_k, int64_t *evals);
int nbmi_get_densities_f64(nbmi_sim *sim, int k, double *rho);
/* What nbmi_compute_colors and nbmi_frame_begin colour by.  NBMI_COLOR_SPEED (the default): the reference's ramp at
 * t = min(speed / max_speed, 1); k and the range are ignored and keep their values, and every handle accepts it.
 * NBMI_COLOR_DENSITY: max_speed is ignored; the call runs the k-NN query above on the handle's stream (enqueued, not
 * waited for; NBMI_ERR_CAPACITY of its build is reported deferred, as a step's is) and colours body i by the same ramp
 * at t = clamp((log10(rho_i) - log10_lo) / (log10_hi - log10_lo), 0, 1); rho = +inf gives t = 1.  nbmi_frame_begin
 * produces exactly nbmi_compute_colors' colours and leaves them where that call leaves them.  Density mode needs
 * log10_hi > log10_lo, both finite, a valid k, and a handle nbmi_knn accepts (else NBMI_ERR_ARG, mode unchanged). */
#define NBMI_COLOR_SPEED 0
#define NBMI_COLOR_DENSITY 1
int nbmi_set_color_mode(nbmi_sim *sim, int mode, int k, double log10_lo, double log10_hi);
int nbmi_get_color_mode(nbmi_sim *sim, int *mode, int *k, double *log10_lo, double *log10_hi); /* outputs may be NULL */

/* ---- friends-of-friends groups --------------------------------------------------------------
 * Of the handle's current float64 state, exactly:
 *   d2(i, j)  as above: (dx dx + dy dy) + dz dz with dx = x_j - x_i, float64 in this association, no FMA.
 *   b2        = link * link, one float64 product computed on the host.
 *   linked    bodies i != j are linked iff d2(i, j) <= b2.  Equality links; a coincident pair (d2 = 0) is linked for
 *             every valid link.
 *   group     a connected component of the link graph; a body without a friend is a group of one.
 *   labels[i] (int32, caller's body order) = the smallest caller index in i's group.  Partition and labels are unique
 *             and independent of any order of evaluation: they equal a brute force's exactly.
 *   n_groups  = the number of distinct labels, singletons included.
 * nbmi_fof: labels, n_groups and evals may each be NULL.  *evals = the number of d2 the call evaluated (a measurement
 * hook like nbmi_knn's).
 * nbmi_fof_catalogue: the groups with members >= min_members (min_members >= 1), ordered by members descending, ties
 * by label ascending.  Per group label, members and 13 doubles {M, c[3], v[3], lo[3], hi[3]}:
 *   M = sum m_j;  c = sum m_j x_j / M;  v = sum m_j v_j / M;  a group with M == 0 has the unweighted means of its
 *   members' positions and velocities instead;  lo / hi = the per-axis min / max of the members' positions (exact).
 * The sums are float64 in a fixed order (no floating-point atomics): two calls on an unchanged state return the same
 * bits.  *count = the number of qualifying groups, which may exceed capacity; at most capacity rows are copied out (the
 * first ones of the order), as nbmi_visible_points does.  label, members and out13 may be NULL when capacity == 0.
 * nbmi_compute_group_colors: one shot, does NOT touch the colour mode; leaves colours where nbmi_compute_colors leaves
 * them (nbmi_get_colors_f32, nbmi_visible_points and nbmi_render_sim see them): a body of a group with members >=
 * min_members gets the speed ramp at t = ((uint32)(label * 2654435761u) >> 8) / 2^24, every other body (0.25, 0.25,
 * 0.25).  It only enqueues; NBMI_ERR_CAPACITY of its build is reported deferred, as a step's is.
 * Refused with NBMI_ERR_ARG, message "<call>: ...": link not finite or <= 0, min_members < 1, capacity < 0, and the
 * handles nbmi_knn refuses (direct N^2, owner mode, a proper shard).  N == 0: success,
 * n_groups = 0, count = 0.  N == 1: one singleton.
 * A call changes nothing that a later step reads (as nbmi_knn).  NBMI_ERR_CAPACITY of the call's own tree build is
 * reported with a step's message.  Quadrupole and leapfrog handles return a plain handle's bits.
 * The first nbmi_fof allocates 16 bytes per body and (shared with nbmi_knn) 32 bytes per node row and 4 bytes per 64
 * bodies; the first catalogue 24 bytes per body more, a radix sort buffer (about 8 bytes per body), 304 bytes per 256
 * bodies and 268 bytes per catalogue row (for the next power of two of rows, at least 1 024; a call that needs more frees
 * the arrays and allocates larger ones). */
int nbmi_fof(nbmi_sim *sim, double link, int32_t *labels /* (N,), may be NULL */, int64_t *n_groups /* may be NULL */,
             int64_t *evals /* may be NULL */);
int nbmi_fof_catalogue(nbmi_sim *sim, double link, int64_t min_members, int64_t capacity, int32_t *label,
                       int64_t *members, double *out13, int64_t *count);
int nbmi_compute_group_colors(nbmi_sim *sim, double link, int64_t min_members);

/* ---- the Euclidean minimum spanning tree of the bodies ---------------------------------------
 * Every friends-of-friends partition at once: the groups at link b are the components left when the tree's edges longer
 * than b are cut, and the N - 1 edge lengths are the merge heights of the single-linkage dendrogram (nbody/mst.py has the
 * host-side consumers).  Of the handle's current float64 state, exactly:
 *   d2(i, j)  as in nbmi_fof: (dx dx + dy dy) + dz dz with dx = x_j - x_i, float64 in this association, no FMA.  It is
 *             symmetric in i and j bit for bit - a negated difference squares to the same value - and the search
 *             evaluates it from either end.
 *   order     the unordered pair {i, j} of caller indices, written with i < j, has the key (d2(i, j), i, j), compared
 *             lexicographically: a strict total order on the N (N - 1) / 2 pairs, ties in d2 included.  A coincident pair
 *             has d2 = 0 and is ordered by its indices.
 *   the tree  the minimum spanning tree of the complete graph under that order.  It is unique: the edge set Kruskal's
 *             algorithm accepts when it takes the pairs in that order, and equally what Prim's or Boruvka's gives when
 *             every comparison uses that order.
 *   output    the N - 1 edges sorted ascending by their key: edge_i[k] < edge_j[k] (int32, caller indices) and
 *             edge_d2[k] = d2 of that pair.  Every value is independent of the key order of the state, of the order of
 *             evaluation and of the handle's history; two calls return the same arrays.
 * Consequences: the number of edges with edge_d2 <= link * link is N - n_groups of nbmi_fof(link), and the components of
 * those edges are exactly nbmi_fof's groups, so the labels obtained from them (the smallest index of a component) equal
 * nbmi_fof's array.
 * edge_i, edge_j, edge_d2, rounds and evals may each be NULL.
 *   *rounds   the number of Boruvka rounds run, at most ceil(log2 N): every round unites every component with at least
 *             one other.
 *   *evals    the number of d2 the call evaluated (a measurement hook like nbmi_fof's).  No wave reads what another
 *             writes during a search, so it is a function of the state: two calls return the same number.
 * N == 0 or 1: success, no edge is written, rounds = 0.
 * Refused with NBMI_ERR_ARG, message "nbmi_mst: ...": the handles nbmi_knn refuses (direct N^2, owner mode, a proper
 * shard).  NBMI_ERR_CAPACITY of the call's own tree build is reported with a step's message (seventy bodies at one
 * position still do not fit).  Coordinates that are not finite leave bodies without a nearest foreign body: NBMI_ERR_HIP,
 * "nbmi_mst: ... rounds left ...".
 * Synchronous, like nbmi_pair_counts_at: errors of earlier steps are reported first, and the call returns with the arrays
 * filled.  It changes nothing that a later step or query reads - state and order, the tree header, the "auto" precision
 * flags, the step count, the stored leapfrog acceleration, the tracers.  Quadrupole and leapfrog handles return a plain
 * handle's arrays.  With nbmi_enable_timers the time from the build's first kernel to the last write - the host's
 * one 16-byte read per round included - goes to "other".
 * The first call allocates 64 bytes per body, 4 bytes per node row, 4 bytes per 2 048 bodies and a radix sort buffer
 * (about 12 bytes per body), and uses - allocating them if no earlier call has - nbmi_fof's 16 bytes per body,
 * nbmi_pair_counts' 4 bytes per node row and (shared with nbmi_knn) 32 bytes per node row and 4 bytes per 64 bodies.  All
 * of it is freed by nbmi_destroy. */
int nbmi_mst(nbmi_sim *sim, int32_t *edge_i /* (N-1,), may be NULL */, int32_t *edge_j /* (N-1,), may be NULL */,
             double *edge_d2 /* (N-1,), may be NULL */, int64_t *rounds /* may be NULL */, int64_t *evals /* may be NULL */);
/* Measurement hook: the rounds of the handle's last nbmi_mst, oldest first, at most `capacity` of them into each array
 * that is not NULL - the d2 evaluated in the round (0 if that call's evals was NULL), the edges it appended, and the
 * host's wall time for it in ms (its kernels and the one read that ends it).  Returns the number of rounds (>= 0; 0
 * before the first call), or a negative error for a bad handle. */
int nbmi_mst_rounds(nbmi_sim *sim, int capacity, int64_t *evals, int64_t *edges, double *ms);

/* ---- exact binned pair counts ---------------------------------------------------------------
 * Of the handle's current float64 state, exactly:
 *   d2(i, j)   as above: (dx dx + dy dy) + dz dz with dx = x_j - x_i, float64 in this association, no FMA.
 *   edges      nb + 1 float64 with 1 <= nb <= 64, all finite, edges[0] >= 0, strictly increasing.
 *   E[k]       = edges[k] * edges[k], one float64 product each, computed on the host.  The E[k] must themselves be finite
 *              and strictly increasing (two close edges may square to one value), else NBMI_ERR_ARG.
 *   below      = the number of unordered pairs i < j with d2(i, j) <= E[0].  With edges[0] == 0 these are the coincident
 *              pairs.
 *   counts[k]  = the number of unordered pairs with E[k] < d2(i, j) <= E[k + 1].  The upper edge belongs to the bin, as
 *              equality links in nbmi_fof: below + counts[0 .. k] is C(edges[k + 1]), the number of pairs within that
 *              distance, and at edges[k + 1] = link it is the number of links of nbmi_fof.
 * The counts are integers summed by integer atomics: the result is unique, independent of any order of evaluation, and
 * equals a brute force's exactly.  counts ((nb,) int64), below, evals and cell_pairs may each be NULL.
 *   *evals      = the number of d2 the call evaluated;
 *   *cell_pairs = the number of pairs it counted through whole cells, without a d2 (a cell of the tree that provably lies
 *              inside one bin as seen from a body adds its body count at once).
 * Both are measurement hooks like nbmi_fof's evals.  N == 0 or N == 1: success, all zeros.
 * Two calls on an unchanged state return the same numbers.  A quadrupole or leapfrog handle returns a plain handle's
 * numbers: the tree is the same.
 * A call changes nothing that a later step reads (state and its order, the tree header - saved and restored -, the
 * "auto" precision flags and force_all64 - the build runs without a dt -, the step count, the stored leapfrog
 * acceleration).  NBMI_ERR_CAPACITY of the call's own tree build is reported with a step's message.
 * Refused with NBMI_ERR_ARG, message "nbmi_pair_counts: ...": nb outside 1 .. 64, null edges, an edge that is not finite,
 * negative or not above the one before it (or whose square is not), and the handles nbmi_knn refuses (direct N^2, owner
 * mode, a proper shard).
 * The first call allocates 4 bytes per node row, 536 bytes of results and (shared with nbmi_knn and nbmi_fof) 32 bytes
 * per node row and 4 bytes per 64 bodies.
 * Environment NBMI_PAIRS_CELLS (read when the handle is created, like the other measurement knobs): 0 never counts a
 * cell whole (pruning stays).  Results are the same; evals, cell_pairs (then 0) and the time are not (DESIGN.md section
 * 4.16 has the A/B). */
int nbmi_pair_counts(nbmi_sim *sim, int nb, const double *edges, int64_t *counts /* (nb,), may be NULL */,
                     int64_t *below /* may be NULL */, int64_t *evals /* may be NULL */, int64_t *cell_pairs /* may be NULL */);

/* ---- exact counts about arbitrary points: DR(r), counts in spheres ---------------------------
 * For each of m arbitrary points, the number of bodies per distance bin.  Of the handle's current float64 state, exactly
 * (the kernel and the tests' NumPy restatement, tests/pairs_at_ref.py, both follow this text):
 *   d2(i, j)          = (dx dx + dy dy) + dz dz with dx = x_j - p_i per component, body j minus point i, float64 in this
 *                     association, no FMA.
 *   edges, E[k]       exactly nbmi_pair_counts': 1 <= nb <= 64, nb + 1 finite float64, edges[0] >= 0, strictly increasing;
 *                     E[k] = edges[k] * edges[k], one float64 product each on the host, finite and strictly increasing.
 *   per_point[i][0]   = the number of bodies j with d2(i, j) <= E[0].
 *   per_point[i][k+1] = the number of bodies j with E[k] < d2(i, j) <= E[k + 1].  The upper edge belongs to the bin.
 *   below, counts[k]  = the sums of column 0 and of column k + 1 over the m points: DR, every (point, body) pair once.
 * Nothing is excluded: a point is not a body, and a point that coincides with a body counts that body in column 0.  With
 * points = nbmi_get_positions_f64, column 0 of row i holds body i itself, its coincident twins and the bodies within
 * edges[0] of it; then counts[k] = 2 nbmi_pair_counts' counts[k] and below = 2 nbmi_pair_counts' below + N.
 * The counts are integers, the totals summed by integer atomics: every value is unique and independent of any order of
 * evaluation, and equals a brute force's exactly.  A point's row does not depend on the other points of the call, on
 * their order or on how the call is split: two calls give the same numbers, duplicated points give identical rows, a
 * permutation of the points permutes the rows.  A quadrupole or leapfrog handle returns a plain handle's numbers.
 * counts ((nb,) int64), below, per_point ((m, nb + 1) int32, row-major), evals and cell_pairs may each be NULL.
 *   *evals      = the number of d2 the call evaluated;
 *   *cell_pairs = the number of (point, body) pairs it counted through whole cells, without a d2.
 * Both are measurement hooks as in nbmi_pair_counts.
 * m == 0: success, counts, below, evals and cell_pairs are zeroed and nothing else is touched.  N == 0: zeros.  N == 1 is
 * served by the tree like every other N (its root is a leaf); nothing is answered on the host.
 * Refused with NBMI_ERR_ARG, message "nbmi_pair_counts_at: ...", before anything is launched and with every output
 * untouched: m < 0, null points_xyz with m > 0, a coordinate that is not finite or exceeds 1e18 in magnitude (the message
 * names the first bad row), nb or edges that nbmi_pair_counts refuses, and the handles nbmi_knn refuses (direct N^2, owner
 * mode, a proper shard).  Points may lie anywhere, outside the root cube too.
 * The call is synchronous.  It changes nothing that a later step or query reads (state and its order, the tree header -
 * saved and restored -, the "auto" precision flags and force_all64 - the build runs without a dt -, the step count, the
 * stored leapfrog acceleration, the tracers and their scratch).  NBMI_ERR_CAPACITY of the call's own tree build is
 * reported with a step's message.
 * The points are processed as nbmi_field_at's - chunks of at most 1 048 576, walked in key order within a chunk of more
 * than 64, NBMI_FIELD_SORT=0 honoured - through nbmi_field_at's scratch (allocated by whichever call comes first), and the
 * tree side is nbmi_pair_counts' (4 bytes per node row, 536 bytes of results, and the shared 32 bytes per node row and 4
 * bytes per 64 bodies).  per_point costs 4 (nb + 1) bytes per row of that scratch more - at most 272 MB, at nb = 64 and
 * a full chunk; the chunk is not made smaller for it - allocated by the first call that asks for per_point, regrown by a
 * call that needs more and freed with the scratch.
 * NBMI_PAIRS_CELLS=0 is honoured as in nbmi_pair_counts: same numbers, cell_pairs == 0. */
int nbmi_pair_counts_at(nbmi_sim *sim, int64_t m, const double *points_xyz /* (m,3) */, int nb,
                        const double *edges /* nb+1 */, int64_t *counts /* (nb,), may be NULL */,
                        int64_t *below /* may be NULL */, int32_t *per_point /* (m, nb+1), may be NULL */,
                        int64_t *evals /* may be NULL */, int64_t *cell_pairs /* may be NULL */);

/* The gravitational field of the handle's current float64 state at m arbitrary points: what a
 * test particle at points_xyz[i] would feel.  The kernels and the tests' NumPy restatement (tests/field_ref.py) both
 * follow this text.  All arithmetic is float64 in the association written, without FMA contraction.
 *
 * Barnes-Hut handle.  The walk is the reference's (nbody/simulation.py:237-274) for a body at p that is not in the tree,
 * over the octree every other call builds for the current positions.  There is no own-leaf rule.  With c the node's
 * centre of mass (a leaf: its body's position), G M its mass times G - both from the build's float64 node rows, the rows
 * nbmi_get_potentials_f64 reads - and half its half size:
 *   d       = c - p per component
 *   dist_sq = ((dx dx + dy dy) + dz dz) + eps^2,   dist = sqrt(dist_sq)
 *   a node is accepted when it is a leaf or (2 half) / dist < theta; otherwise it is opened;
 *   an accepted node is applied only when G M > 0 and dist_sq > eps^2: a point that coincides with a body gets nothing
 *   from that body's leaf - the rule the force and potential walks have for coincident bodies;
 *   an applied node adds   acc += d * (G M / (dist * dist_sq)),   phi -= G M / dist.
 * terms[i] = the number of nodes applied to point i.
 * In quadrupole mode (nbmi_set_multipole) an applied internal cell also carries the second-order terms, evaluated in
 * float64 from the cell's float64 second moments P about its centre of mass (G folded in), with u = dist_sq:
 *   phi += 1/2 [tr P u^-3/2 - 3 (d^T P d) u^-5/2]
 *   acc += [7.5 (d^T P d) u^-7/2 - 1.5 tr P u^-5/2] d - 3 u^-5/2 P d
 * terms is the same in both modes.
 * Direct handle.  The exact sum over all N bodies with the same two formulas (G M = G m_j, c = x_j) and the one guard
 * dist_sq > eps^2; terms[i] = the number of bodies applied.
 *
 * Fixed summation order.  Each point sums its terms in pre-order of the node array (direct: in body order).  A point's
 * result does not depend on the other points of the call, on their order or on how the call is split: two calls give the
 * same bits, duplicated points give identical rows, a permutation of the points permutes the rows.
 * Consequences (tested bit for bit, monopole and quadrupole), Barnes-Hut: the accepted set at a body's own position is
 * that body's set, so with points = nbmi_get_positions_f64, phi equals nbmi_get_potentials_f64 and the sum of terms
 * equals nbmi_diagnostics' terms.
 *
 * acc_xyz ((m,3)), phi ((m,)) and terms ((m,) int32) may each be NULL.  m == 0: success, nothing is touched.  N == 0:
 * zeros.  NBMI_ERR_ARG, message "nbmi_field_at: ...": m < 0, null points_xyz with m > 0, a coordinate that is not finite
 * or exceeds 1e18 in magnitude (the message names the first bad row), owner-mode handles and handles with a proper shard.
 * Points may lie anywhere, outside the root cube too.
 * A call changes nothing that a later step reads (state and its order, the tree header - saved and restored -, the
 * "auto" precision flags and force_all64 - the build runs without a dt -, the step count, the stored leapfrog
 * acceleration): a leapfrog handle returns a plain handle's bits.  NBMI_ERR_CAPACITY of the call's own tree build is
 * reported with a step's message.
 * The points are processed in chunks of at most 1 048 576; within a chunk of more than 64 points they are walked in the
 * order of their octant keys in the tree's root cube (outside coordinates clamped to its faces) - speed only, see the
 * fixed order above.  Scratch: 108 bytes per point of the largest chunk so far plus the sort's temp buffer for that many
 * (key, index) pairs - at most 113 MB and that buffer, however large m is - and, shared with nbmi_get_potentials_f64, 32
 * bytes per node row.  Uploads and downloads go chunk by chunk through that scratch.
 * Environment NBMI_FIELD_SORT (read when the handle is created, like the other measurement knobs): 0 walks the points
 * in the caller's order.  Results are the same; the time is not. */
int nbmi_field_at(nbmi_sim *sim, int64_t m, const double *points_xyz /* (m,3) */,
                  double *acc_xyz /* (m,3), may be NULL */, double *phi /* (m,), may be NULL */,
                  int32_t *terms /* (m,), may be NULL */);

/* The tidal tensor T_ab = d a_a / d x_b = -d^2 phi / dx_a dx_b of the handle's current float64 state, at m arbitrary
 * points (nbmi_tidal_at) and at every body's own position (nbmi_get_tidal_f64); DESIGN.md section 4.27.  |T|^-1/2 is the
 * local dynamical time and the eigenvalues of -T are the squared frequencies an integrator has to follow.  The kernels
 * and the tests' NumPy restatement (tests/tidal_ref.py) both follow this text.  All arithmetic is float64 in the
 * association written, without FMA contraction, sqrt and divide correctly rounded.
 * tidal6 rows are {Txx, Tyy, Tzz, Txy, Txz, Tyz}: the order of nbmi_get_cell_moments.
 *
 * Accepted set.  Exactly the same accepted set as nbmi_field_at for the same point: the same octree of the current
 * positions, the same opening test ((2 half) / dist < theta, with its fp32 band and its float64 re-decision), no own-leaf
 * rule, and an accepted node is applied only when G M > 0 and dist_sq > eps^2.  terms[i] is therefore the number
 * nbmi_field_at returns for the point, in both multipole modes.
 * Monopole term.  With d = c - p, u = dist_sq = ((dx dx + dy dy) + dz dz) + eps^2 and dist = sqrt(u) as in nbmi_field_at,
 * an applied node adds
 *   w  = G M / (dist * u)                (nbmi_field_at's w)
 *   w5 = (3.0 * w) / u
 *   T_aa += (d_a * d_a) * w5 - w
 *   T_ab += (d_a * d_b) * w5             (a != b)
 * which is G M [3 d d^T u^-5/2 - I u^-3/2].  Its trace is -3 G M eps^2 u^-5/2: zero for eps == 0, and -4 pi G times the
 * Plummer density otherwise.
 * Quadrupole mode.  An applied internal cell (leaves add nothing) also adds the second-order term, from the cell's
 * float64 second moments P about its centre of mass (G folded in; the rows nbmi_field_at reads).  With
 *   g_x = (Pxx dx + Pxy dy) + Pxz dz,  g_y = (Pxy dx + Pyy dy) + Pyz dz,  g_z = (Pxz dx + Pyz dy) + Pzz dz      (g = P d)
 *   q   = (dx (Pxx dx + 2.0 (Pxy dy + Pxz dz)) + dy (Pyy dy + 2.0 (Pyz dz))) + dz (Pzz dz)                      (d^T P d)
 *   tr  = (Pxx + Pyy) + Pzz
 *   i5  = ((1.0 / dist) / u) / u,   i7 = i5 / u,   i9 = i7 / u
 *   A = (1.5 * tr) * i5 - (7.5 * q) * i7     B = (52.5 * q) * i9 - (7.5 * tr) * i7     C = 3.0 * i5     D = 15.0 * i7
 * it adds, as one number per component,
 *   T_aa += ((A + B * (d_a * d_a)) + C * P_aa) - D * (g_a * d_a + d_a * g_a)
 *   T_ab += (B * (d_a * d_b) + C * P_ab) - D * (g_a * d_b + d_a * g_b)                                          (a != b)
 * after the node's monopole term.  Both parts are minus the Hessian of what nbmi_field_at adds to phi.
 * Direct handle.  The exact sum over all N bodies in body order with the monopole term (G M = G m_j, c = x_j) and the one
 * guard dist_sq > eps^2; terms[i] = the number of bodies applied.
 *
 * Fixed summation order.  Each point sums its terms in pre-order of the node array (direct: in body order).  A row does
 * not depend on the other points of the call, on their order or on how the call is split: two calls give the same bits,
 * duplicated points give identical rows, a permutation of the points permutes the rows.
 *
 * nbmi_get_tidal_f64: the same tensor at every body's own position, without an upload, rows in the caller's body order:
 * nbmi_get_potentials_f64's walk (a body in the lane, the build's band; the body's own leaf has d = 0 and is dropped by
 * the guard).  tidal6 equals nbmi_tidal_at at nbmi_get_positions_f64 bit for bit, monopole and quadrupole, and the
 * per-body term count equals the potential's.  Direct handles are accepted: a body's own term is skipped by the guard.
 *   norm[i] = sqrt(((Txx^2 + Tyy^2) + Tzz^2) + 2.0 * ((Txy^2 + Txz^2) + Tyz^2)),  the Frobenius norm of row i.
 *
 * tidal6, terms and norm may each be NULL.  m == 0: success, nothing is touched.  N == 0: zeros (nbmi_get_tidal_f64:
 * nothing to write).  NBMI_ERR_ARG, message "nbmi_tidal_at: ..." or "nbmi_get_tidal_f64: ...": m < 0, null points_xyz with
 * m > 0, a coordinate that is not finite or exceeds 1e18 in magnitude (the message names the first bad row), owner-mode
 * handles and handles with a proper shard.
 * A call changes nothing that a later step or query reads (state and its order, the tree header - saved and restored -,
 * the "auto" precision flags and force_all64, the step count, the stored leapfrog acceleration, the tracers): a leapfrog
 * handle returns a plain handle's bits.  NBMI_ERR_CAPACITY of the call's own tree build is reported with a step's message.
 * nbmi_tidal_at processes the points as nbmi_field_at does - chunks of at most 1 048 576, walked in key order within a
 * chunk of more than 64, NBMI_FIELD_SORT=0 honoured: same bits, other time - through nbmi_field_at's scratch.
 * Memory: the tensor rows cost 48 bytes per row of that scratch on top of its 108 (at most 50 MB), allocated by the
 * first nbmi_tidal_at and freed with the scratch.  nbmi_get_tidal_f64 allocates nothing: its 56 bytes per body (6 + 1
 * doubles) are the getters' staging buffer, which every handle has. */
int nbmi_tidal_at(nbmi_sim *sim, int64_t m, const double *points_xyz /* (m,3) */,
                  double *tidal6 /* (m,6), may be NULL */, int32_t *terms /* (m,), may be NULL */);
int nbmi_get_tidal_f64(nbmi_sim *sim, double *tidal6 /* (N,6), caller's body order, may be NULL */,
                       double *norm /* (N,), may be NULL */);

/* Massless tracer particles carried by the handle's integrator: m test particles that feel the
 * bodies and pull on nothing.  They appear in no tree, no body getter, no diagnostic, no frame and no colour pass; the
 * bodies' trajectories, nbmi_force_precision_share, the walk counters and every query are bit for bit what they are on
 * a handle without tracers.  The kernels and the tests' NumPy replay (tests/tracer_ref.py) both follow this text.
 *
 * Field.  In every substep a tracer at p is accelerated by a = F(p), exactly nbmi_field_at's acc for the point p: the
 * octree of the bodies' positions at which that substep evaluates its forces, the handle's theta, eps and multipole mode,
 * float64 without FMA, sums in pre-order of the node array (direct handles: the exact sum in body order).
 * Integration.  The handle's integrator (nbmi_set_integrator), float64 without FMA, per component, as written:
 *   kick-drift:  a = F(p) on the tree of x_n;  v = (v + a * dt) * damping;  p = p + v * dt.
 *   leapfrog, h = 0.5 * dt:  v = v + a * h;  p = p + v * dt;  a = F(p) on the tree of the drifted bodies;
 *                v = (v + a * h) * damping.
 * The leapfrog's stored a costs 24 bytes per tracer, allocated by the first leapfrog step with tracers.  It is dropped
 * and primed again (a = F(p), inside the next step, state untouched) whenever the bodies' stored acceleration is - after
 * nbmi_create, nbmi_set_state, a switch of integrator or multipole order, a reported NBMI_ERR_CAPACITY - and after
 * nbmi_set_tracers.
 * Retired tracers.  A tracer whose row holds a value that is not finite, or a position coordinate beyond 1e18 in
 * magnitude, when a kernel of a substep reaches it is not walked by that kernel and its row stays as it is.  Kick-drift
 * has one such kernel per substep, so the row of a retired tracer is the one its last whole substep left.  Leapfrog has
 * two, the opening half-kick and drift and the closing walk: a tracer whose drift carries it beyond 1e18 retires in the
 * middle of that substep - it keeps the drifted position and the half-kicked velocity, gets no closing half-kick and no
 * new stored a - and stays so from then on.
 * On a leapfrog handle the tracers' opening half-kick and drift are enqueued after the substep's octree build (the
 * bodies' come before it): the tracers are updated in place, and a build that does not fit must find them untouched.
 * Errors.  A substep whose octree did not fit advances neither bodies nor tracers.
 * N == 0: a = 0, the tracers move on straight lines.  nbmi_set_state leaves the tracers where they are.
 *
 * nbmi_set_tracers replaces all tracers by m new ones (it waits for the work enqueued so far); m == 0 removes them and
 * frees their arrays.  velocities_xyz == NULL: zero velocities.  NBMI_ERR_ARG, message "nbmi_set_tracers: ...": m < 0,
 * m above 67 108 864 (2^26, the largest m accepted), null positions_xyz with m > 0, a position coordinate that is not
 * finite or exceeds 1e18 in magnitude, a velocity that is not finite (the message names the first bad row), owner-mode
 * handles and handles with a proper shard; nbmi_set_shard in turn refuses a proper shard while tracers exist.  A refused
 * call leaves the tracers as they were.
 * Memory: 48 bytes per tracer of state (positions and velocities, (m,3) float64 in the caller's order) and, on a
 * Barnes-Hut handle, 48 bytes per tracer of one chunk - min(m, 1 048 576) rows - of scratch that belongs to the tracers
 * (columns in walk order, sort keys and indices in and out), the sort's temp buffer for that many pairs and, shared with
 * nbmi_get_potentials_f64, 32 bytes per node row.  A step walks the tracers chunk by chunk, each chunk of more than 64
 * in the order of its octant keys in the step's root cube (NBMI_FIELD_SORT=0: in the caller's order) - speed only - and
 * never waits for the host.  A handle without tracers enqueues and allocates what it did before.
 *
 * nbmi_tracer_count: m (-1 for a null handle).  nbmi_get_tracers_f64: rows in the caller's order, either pointer may be
 * NULL; it waits for the steps enqueued and reports their errors as the body getters do.  nbmi_get_tracer_positions_f32
 * rounds the float64 positions to float32 on the host.  With no tracers the getters touch nothing. */
int nbmi_set_tracers(nbmi_sim *sim, int64_t m, const double *positions_xyz /* (m,3) */,
                     const double *velocities_xyz /* (m,3), may be NULL */);
int64_t nbmi_tracer_count(nbmi_sim *sim);
int nbmi_get_tracers_f64(nbmi_sim *sim, double *positions_xyz /* (m,3), may be NULL */,
                         double *velocities_xyz /* (m,3), may be NULL */);
int nbmi_get_tracer_positions_f32(nbmi_sim *sim, float *positions_xyz /* (m,3) */);

/* ---- mass and velocity fields on a regular grid --------------------------------------------
 * Deposits the handle's current float64 state on a grid of dims[0] x dims[1] x dims[2] cells that covers [lo, hi) per
 * axis: surface-density maps (a dims of 1 projects along that axis), density cubes, and the planes that mean-velocity and
 * dispersion maps are made of.  `quantities` selects the planes, in the order of the bits: P is their number (at most 6).
 * Masses are m, not G m, as in nbmi_knn.  Velocities are read as stored: the reference's kick-drift keeps them half a step
 * apart from the positions (as in nbmi_diagnostics); a leapfrog handle's are synchronized.
 *
 * This text is the specification; the kernels and the tests' NumPy restatement (tests/deposit_ref.py) both follow it.
 * All arithmetic is float64 in the association written, without FMA contraction.  Per call:
 *   Grid constants.  inv_a = (double) dims_a / (hi_a - lo_a) per axis, computed once on the host.
 *   Quantum of a plane.  mx = the maximum of |q_j| over ALL N bodies, inside the grid or not (a maximum is exact in any
 *     order).  mx == 0 (or N == 0): the plane is zeros and its exponent reads 0.  Otherwise, with frexp(mx) = (f, E) and
 *     L = the bit length of N, the exponent is e = E + L - 62, so that |k_j| <= 2^(62 - L) + 0.5 and, with N < 2^L, every
 *     cell's integer sum stays inside int64.  exponents[p] = e.
 *   Position on an axis.  u_a = (x_a - lo_a) * inv_a.  A body with a coordinate that is not finite is skipped and counted
 *     in stats3[2].
 *   NGP (nearest grid point), and any axis with dims_a == 1 under either scheme: i_a = floor(u_a) with weight 1.  (A
 *     projection is asked for with dims_a == 1; CIC on such an axis would drop half of every body.)
 *   CIC (cloud in cell), on an axis with dims_a >= 2: s = u_a - 0.5, i = floor(s), f = s - i; cell i gets the weight
 *     1.0 - f and cell i + 1 the weight f.
 *   Which cells take part.  A cell index takes part only if 0 <= i < dims_a, compared on the floored double (i + 1 is
 *     that double plus 1.0) before any conversion to an integer.  The rest is dropped: no wrap-around, no clamping.
 *   One contribution.  A (body, cell) pair whose three indices all take part - a weight of 0 included - with the weights
 *     wx, wy, wz is c = q * ((wx * wy) * wz); its integer is k = (int64) rint(ldexp(c, -e)), to nearest, ties to even.
 *   Output.  K[plane][cell] = the sum of k over all contributions, an exact integer sum (64-bit integer atomics);
 *     out = ldexp((double) K, e).  stats3 = {bodies with at least one contribution, contributions applied, bodies skipped
 *     as not finite}.
 * Consequences (tested):
 *   The result does not depend on the order of the state rows, on the handle type (Barnes-Hut or direct N^2) or on how
 *   the kernel aggregates; two calls give the same bits.
 *   The NUMBER plane under NGP holds exact counts, and its cell sum equals stats3[0].
 *   |out - exact sum of c| <= 0.5 * 2^e * (contributions of that cell), plus one rounding of the final conversion.
 *   The price of exactness: a body whose |q| is below 2^(e - 1) contributes nothing - about 2^-36 of the largest body at
 *   2^26 bodies.
 * NBMI_ERR_ARG, message "nbmi_deposit: ...", before anything is launched and with `out` untouched: null lo, hi, dims or
 * out; a bound that is not finite; hi_a <= lo_a, or hi_a - lo_a or inv_a not finite; dims_a < 1; P * cells > 2^28; a scheme
 * other than 0 or 1; quantities equal to 0 or with unknown bits; owner-mode handles and handles with a proper shard.
 * After the pass over the maxima, `out` still untouched: a selected quantity whose maximum is not finite (the message
 * names the plane).  Barnes-Hut and direct handles are accepted; no tree is built.  N == 0 gives zeros.
 * A call changes nothing that a later step or query reads (the state and its order, the tree header, the precision flags,
 * the step count, the stored leapfrog acceleration, the tracers).  It waits for the work enqueued so far and reports
 * deferred errors as the getters do.  Scratch: 8 * P * cells bytes on the device, kept and grown on demand, and 72 bytes of
 * results.  With nbmi_enable_timers the device time of the call's kernels (without its copies) is added to "other".
 * Environment NBMI_DEPOSIT_AGG (read when the handle is created, like the other measurement knobs): 1 = the lanes of a
 * workgroup that hit the same cell are combined in LDS first and one atomic leaves per distinct cell, 0 = one global
 * atomic per contribution.  The results are the same bits; the time is not (DESIGN.md section 4.20 has the A/B). */
#define NBMI_DEPOSIT_NGP 0
#define NBMI_DEPOSIT_CIC 1
#define NBMI_DEPOSIT_NUMBER 1   /* 1 plane:  q = 1                                   */
#define NBMI_DEPOSIT_MASS 2     /* 1 plane:  q = m                                   */
#define NBMI_DEPOSIT_MOMENTUM 4 /* 3 planes: q = m * vx, m * vy, m * vz              */
#define NBMI_DEPOSIT_KINETIC 8  /* 1 plane:  q = m * ((vx*vx + vy*vy) + vz*vz)       */
int nbmi_deposit(nbmi_sim *sim, const double lo[3], const double hi[3], const int32_t dims[3], int scheme,
                 int quantities, double *out /* (P, dims[2], dims[1], dims[0]) C order */,
                 int64_t *stats3 /* may be NULL */, int32_t *exponents /* (P,), may be NULL */);

/* ---- radial profiles and mass radii about a centre --------------------------------------------
 * nbmi_deposit's spherical counterpart: sums of per-body quantities over the shells between nb + 1 radii about `center`,
 * and the squared radii that hold given fractions of the mass (Lagrangian radii).  Masses are m, not G m; velocities are
 * read as stored (see nbmi_deposit).  Both calls accept Barnes-Hut and direct handles, build no tree, refuse owner-mode
 * handles and handles with a proper shard, wait for the work enqueued so far and report deferred errors as the getters
 * do, and change nothing that a later step or query reads (the state and its order, the tree header, the precision flags,
 * the step count, the stored leapfrog acceleration, the tracers).  With nbmi_enable_timers the device time of their
 * kernels (without the copies) is added to "other".
 *
 * This text is the specification; the kernels and the tests' NumPy restatement (tests/profile_ref.py) both follow it.
 * All arithmetic is float64 in the association written, without FMA contraction; sqrt and divide are correctly rounded.
 *
 * nbmi_radial_profile.  `quantities` selects the planes, in the order of the bits: P is their number (at most 8).
 *   Edges.  1 <= nb <= 256; edges[0 .. nb] finite, edges[0] >= 0, strictly increasing; E[k] = edges[k] * edges[k], one
 *     host product each, must again be finite and strictly increasing.
 *   Per body.  r_a = x_a - center_a and w_a = v_a - bulk_velocity_a, one subtraction each (bulk_velocity == NULL: w = v
 *     and no subtraction is made).  r2 = (rx rx + ry ry) + rz rz.  A body whose r2 is not finite is skipped: it is counted
 *     in stats3[2] and takes no part in anything below, the maxima included.
 *   Slot.  s = the number of k in 0 .. nb with E[k] < r2.  s == 0 is the inner ball r2 <= E[0] (with edges[0] == 0: the
 *     bodies exactly at the centre); 1 <= s <= nb is the shell E[s-1] < r2 <= E[s], the upper edge belongs to the shell;
 *     s == nb + 1 is beyond: the body contributes nothing and is counted in stats3[1].
 *   Quantities.  rho = sqrt(r2);  vr = ((rx wx + ry wy) + rz wz) / rho, and vr = 0 when rho == 0;
 *     w2 = (wx wx + wy wy) + wz wz.  The q of the planes are listed at the NBMI_PROFILE_ constants below; in
 *     ANGULAR_MOMENTUM each product is rounded, then the difference, then the product by m.
 *   Quantum of a plane (nbmi_deposit's rule).  mx = the maximum of |q_j| over all bodies that are not skipped, in a slot
 *     or beyond.  mx == 0 (or N == 0): the plane is zeros and its exponent reads 0.  Otherwise, with frexp(mx) = (f, Ex)
 *     and L = the bit length of N, e = Ex + L - 62.  exponents[p] = e.
 *   Contribution and output.  k = (int64) rint(ldexp(q, -e)), ties to even; K[plane][slot] = the exact integer sum over
 *     the bodies of the slot; out[plane][slot] = ldexp((double) K, e) for the slots 0 .. nb.  stats3 = {bodies in a slot,
 *     bodies beyond, bodies skipped}; their sum is N.
 *   Consequences (tested): the result does not depend on the order of the state rows, on the handle type or on how the
 *   kernel aggregates; two calls give the same bits; the NUMBER plane holds exact counts and its sum equals stats3[0];
 *   |out - exact sum of q| <= 0.5 * 2^e * (bodies of the slot) plus one rounding of the final conversion.
 *   NBMI_ERR_ARG, message "nbmi_radial_profile: ...", before anything is launched and with `out` untouched: null center,
 *   edges or out; a centre or bulk velocity that is not finite; nb outside 1 .. 256; a bad edge (the message names its
 *   index and value); quantities equal to 0 or with unknown bits; the handles above.  After the pass over the maxima,
 *   `out` still untouched: a selected plane whose maximum is not finite (the message names the plane).  N == 0 gives zeros.
 *   Scratch: 16.5 KB on the device (8 maxima, 3 stats, 8 x 257 sums), allocated by the first call.
 *   A workgroup adds its 2 048 bodies' integers into a table in LDS, one LDS atomic per body and plane, and the table
 *   leaves as one global atomic per non-zero (slot, plane).  There is no environment knob: the alternative that was
 *   measured, a wave summing its lanes of equal slot first, is scripts/experiments/profile_wave_sum.patch (DESIGN.md
 *   section 4.26 has the A/B).
 *
 * nbmi_mass_radii.  r2 and the skip rule are as above; stats2 = {bodies taking part, bodies skipped}.
 *   Mass quantum.  mx = the largest mass over all N bodies; with frexp(mx) = (f, Ex) and L = the bit length of N,
 *     e = Ex + L - 53 (mx == 0 or N == 0: e = 0) and k_j = (int64) rint(ldexp(m_j, -e)), so that K_total = the sum of k_j
 *     over the bodies taking part is < 2^53: it and every partial sum convert to float64 exactly.  *exponent = e.  This
 *     quantum is deliberately NOT the profile's MASS plane's (e = Ex + L - 62): there the sums only have to fit int64,
 *     here the threshold below is a float64 product with K_total, which must be exact in float64.
 *   Selection.  1 <= nf <= 64 fractions, each finite with 0 < f <= 1, in any order, repeats allowed.  Per fraction
 *     T = max(1, (int64) ceil(f * (double) K_total)), one product and one ceil.  radius2[f] = the smallest value R among
 *     the r2 of the bodies taking part for which the sum of k_j over the bodies with r2_j <= R is >= T;  inside[f] = the
 *     number of bodies taking part with r2_j <= R;  mass_inside[f] = ldexp((double) that sum, e);
 *     *total_mass = ldexp((double) K_total, e).  Bodies of equal r2 enter together, so the result is unique whatever
 *     order ties are met in.  K_total == 0 (N == 0, all masses below the quantum, nobody taking part): success with
 *     radius2 = NaN, inside = 0, mass_inside = 0 and total_mass = 0.
 *   NBMI_ERR_ARG, message "nbmi_mass_radii: ...", before anything is launched and with the outputs untouched: null center,
 *   fractions or radius2; a centre that is not finite; nf outside 1 .. 64; a fraction outside (0, 1] or not finite; the
 *   handles above.  After the pass over the masses, the outputs still untouched: a mass that is negative or not finite.
 *   Device path: (bits of r2, row) pairs - a non-negative finite double orders as its bits, a skipped body gets a key
 *   above all of them - through the library's radix sort, a segmented prefix sum of k in sorted order, and one test
 *   "last of its tie run and C_prev_run < T <= C_run" per run and fraction.  Nothing of O(N) crosses to the host.
 *   Scratch: 32 bytes per body (keys and rows in and out of the sort, k in sorted order), the sort's temp buffer for N
 *   pairs (12 bytes per body and its status rows), 24 bytes per 2 048 bodies and 1.6 KB of results; allocated by the
 *   first call (N is fixed), freed by nbmi_destroy. */
#define NBMI_PROFILE_NUMBER 1            /* 1 plane:  q = 1                                           */
#define NBMI_PROFILE_MASS 2              /* 1 plane:  q = m                                           */
#define NBMI_PROFILE_RADIAL_MOMENTUM 4   /* 1 plane:  q = m * vr                                      */
#define NBMI_PROFILE_RADIAL_KINETIC 8    /* 1 plane:  q = (m * vr) * vr                               */
#define NBMI_PROFILE_KINETIC 16          /* 1 plane:  q = m * w2                                      */
#define NBMI_PROFILE_ANGULAR_MOMENTUM 32 /* 3 planes: q = m * (ry wz - rz wy), m * (rz wx - rx wz), m * (rx wy - ry wx) */
int nbmi_radial_profile(nbmi_sim *sim, const double center[3], const double bulk_velocity[3] /* NULL = 0 */, int nb,
                        const double *edges /* nb+1 */, int quantities, double *out /* (P, nb+1) C order */,
                        int64_t *stats3 /* may be NULL */, int32_t *exponents /* (P,), may be NULL */);
int nbmi_mass_radii(nbmi_sim *sim, const double center[3], int nf, const double *fractions /* nf */,
                    double *radius2 /* (nf,) */, int64_t *inside /* (nf,), may be NULL */,
                    double *mass_inside /* (nf,), may be NULL */, double *total_mass /* may be NULL */,
                    int64_t *stats2 /* may be NULL */, int32_t *exponent /* may be NULL */);

/* Multi-GPU (one process per GPU).  A handle created with nbmi_create holds ALL bodies; with a
 * shard set, step() integrates only the key-sorted ranks [begin,end) (direct method: the body
 * indices [begin,end), its state is never re-ordered) and leaves the others untouched until
 * nbmi_import_ranks() supplies them.  Packed row = 8 doubles
 * {x,y,z,vx,vy,vz,m,id}.  Pointers are DEVICE pointers (e.g. torch tensors' data_ptr()) so the
 * exchange itself can be an RCCL all-gather issued by the host framework.  Results equal the unsharded
 * handle's bit for bit when `begin` is a multiple of 64 (a wave's 64 bodies, and with them the order of its
 * fp32 sums, are then the same however the ranks are cut; nbody/sharded.py::shard_bounds does that).  The rows carry
 * every body's OWN mass: masses are fixed at creation (a direct-N^2 handle whose bodies all have the same mass takes
 * G m out of its pair loop, decided once at nbmi_create; at softening 0, or one so small that the fp32 G m eps^-3 of a
 * j == i term overflows, both methods skip the pairs with dist_sq <= eps^2 instead, coincident bodies included). */
int nbmi_set_shard(nbmi_sim *sim, int64_t begin, int64_t end);
int nbmi_export_shard(nbmi_sim *sim, void *dev_rows);                              /* (end-begin, 8) f64 */
int nbmi_import_ranks(nbmi_sim *sim, const void *dev_rows, int64_t begin, int64_t end);

/* Multi-GPU stage 2, "owner mode" (BASELINE north_star: bodies shard by Morton range, exchange of the upper /
 * locally essential octree cells).  A rank's handle holds only the bodies whose octant key falls into the
 * rank's key range (rebalanced every step), builds the octree of THOSE bodies inside the GLOBAL root cube
 * (compute_bounds over the whole system, simulation.py:308-317) and walks its own tree plus, behind it in the
 * same node array, the part of every other rank's tree that some body of this rank can open (the other ranks
 * prune their trees against this rank's bounding boxes with the reference's own opening test, made conservative
 * by 1e-9).  Per-rank sort / build / memory no longer grow with the number of ranks.  [r3] The ranks' trees are
 * pieces of ONE global octree: every rank publishes a small table about its first and last bodies
 * (nbmi_owner_chain_doubles() doubles, written by nbmi_owner_adopt, all-gathered like the boxes), and
 * nbmi_owner_export_let first turns the own tree into the rank's piece of the global pre-order node array - cells
 * that reach into higher ranks get the global moments, cells that exist only across a boundary are inserted, the
 * copies of cells that begin on a lower rank are dropped.  nbmi_owner_step puts the received pieces around the own
 * one in rank order.  Every body then visits the single-GPU run's accepted nodes in the single-GPU order: with
 * float64 forces the result equals the single handle's to rounding (tests: 1e-13 after 4 steps), in the default
 * "auto" precision 1 M bodies on 8 ranks stay within 1.4e-5 of the float64 reference after 100 steps.
 * The replicated-tree exchange above (nbmi_set_shard) stays as the bit-for-bit mode.
 *
 * One step, host side (buffers are DEVICE pointers; the collectives are the host framework's):
 *   nbmi_owner_maxabs(h, m)                         m <- max |coordinate| of the owned bodies (1 double)
 *        all-reduce MAX of m
 *   nbmi_owner_sample(h, m, samples, S, V)          keys of the owned bodies in the global cube; V <= S regular samples
 *                                                   (the other slots all ones = ignored).  V in proportion to the rank's
 *                                                   body count, e.g. 0.8 S n_rank world / n_total, keeps the ranks balanced
 *        all-gather of the samples                  (world x S keys)
 *   nbmi_owner_partition(h, all, world*S, send, counts)   splitters at equal quantiles; rows {x,y,z,vx,vy,vz,m,id} of
 *                                                   the bodies that now belong to ANOTHER rank, grouped by destination
 *                                                   in `send`; counts[world] on the host (counts[own rank] = 0)
 *        all-to-all of the counts, all-to-all-v of the rows  (only bodies that crossed a splitter travel)
 *   nbmi_owner_adopt(h, recv, n_recv, m, box, chain)   the n_recv received rows join the bodies that stayed: keys, sort, octree;
 *                                                   box <- B = nbmi_owner_boxes_per_rank() bounding boxes (6 doubles
 *                                                   each: lo xyz, hi xyz) of the bodies inside cells of the own
 *                                                   tree (level 4, refined to level 11 along the two boundary
 *                                                   chains), in key order; unused boxes are empty (lo > hi)
 *                                                   chain <- the rank's boundary table (nbmi_owner_chain_doubles() doubles)
 *        all-gather of the boxes, all-gather of the tables   (world x B x 6 doubles, world x C doubles)
 *   nbmi_owner_export_let(h, boxes, chains, let, counts)   the own tree becomes the rank's piece of the global tree, then is
 *                                                   pruned against EACH other rank's boxes: counts[j] rows
 *                                                   for rank j, packed one destination after the other in `let`
 *                                                   (rows of nbmi_owner_let_row_bytes() = 48 bytes, float64
 *                                                   throughout: {cx, cy, cz, G m, float s2t, link, node index, level};
 *                                                   let_capacity rows in all); counts[world] on the host
 *        all-to-all of the counts, all-to-all-v of the rows
 *   nbmi_owner_step(h, recv, recv_counts, dt)       put the received pieces (packed in rank order, at most
 *                                                   let_capacity rows) around the own one, walk, kick-drift
 *
 * Host waits [r3]: with nbmi_set_exchange_sync(h, 0) and the collectives enqueued ON the handle's stream
 * (nbmi_stream; torch.cuda.ExternalStream), nbmi_owner_maxabs / _sample / _adopt / _step only enqueue; the two
 * calls that hand counts to the host wait once each (nbmi_owner_partition, nbmi_owner_export_let).  With the
 * default sync = 1 every call waits for its own work, as in round 2.  World size 1 skips the splitter, dead-row
 * and box work altogether.
 *
 * Force precision [r3]: an owner handle computes forces like a plain one (nbmi_set_force_precision; default
 * "auto") - the exchanged rows carry the float64 centre of mass and G m of every node, and the receiver builds
 * both walk records from them.  "auto" is decided while nbmi_owner_adopt builds the tree, so the dt of the
 * step has to be known by then: nbmi_owner_set_dt(h, dt) before nbmi_owner_adopt (no dt set: fp32 forces, as
 * "auto" does for any build that is not part of a step).  Each rank decides for its own waves by their density;
 * the "most of the system asks => every wave" half of the rule is taken SYSTEM-WIDE [r4]: after
 * nbmi_owner_export_let, nbmi_owner_step_facts gives the rank's votes (asking waves, waves), the caller sums them
 * over the ranks (they ride in the exchange of the tree counts), applies the single handle's rule (enter above a third,
 * leave below a quarter) and hands the verdict to every rank with nbmi_owner_set_all64 before nbmi_owner_step - the
 * arithmetic no longer depends on the world size or on where the splitters fall.  Without a verdict (-1, default) a
 * rank applies the rule to its own waves.
 *
 * Getters of an owner handle return the owned bodies in their current (key) order; nbmi_owner_get_ids gives the
 * global body ids of those rows. */
nbmi_sim *nbmi_create_owner(int64_t n, const double *positions_xyz, const double *velocities_xyz, const double *masses,
                            const int32_t *global_ids, int64_t capacity, int64_t let_capacity, int world, int rank,
                            double G, double softening, double damping, double theta, int device);
int64_t nbmi_owner_count(nbmi_sim *sim);
int nbmi_owner_boxes_per_rank(void);
int nbmi_owner_let_row_bytes(void);
int nbmi_owner_set_dt(nbmi_sim *sim, double dt);
int nbmi_owner_get_ids(nbmi_sim *sim, int32_t *out);
int nbmi_owner_maxabs(nbmi_sim *sim, void *dev_maxabs);
int nbmi_owner_sample(nbmi_sim *sim, const void *dev_maxabs, void *dev_samples, int nsamples, int nvalid);
int nbmi_owner_partition(nbmi_sim *sim, const void *dev_all_samples, int total_samples, void *dev_send_rows,
                         int64_t *counts_host);
int nbmi_owner_chain_doubles(void);
int nbmi_owner_adopt(nbmi_sim *sim, const void *dev_recv_rows, int64_t n_recv, const void *dev_maxabs, void *dev_boxes,
                     void *dev_chain);
int nbmi_owner_export_let(nbmi_sim *sim, const void *dev_boxes, const void *dev_chains, void *dev_let, int64_t *counts_host);
int nbmi_owner_step(nbmi_sim *sim, const void *dev_recv_let, const int64_t *recv_counts_host, double dt);
/* After nbmi_owner_export_let: out4 = {waves of this rank whose own density asks for float64 forces, waves of this
 * rank (both 0 unless the mode is "auto" and a dt is set), tree rows that still fit in front of the own piece of the
 * walk array, tree rows that fit behind it} - what every rank needs to know of every other rank to take the
 * system-wide precision decision and to evaluate nbmi_owner_step's "received trees do not fit" for all ranks
 * together (a rank raising alone leaves the others in the next collective). */
int nbmi_owner_step_facts(nbmi_sim *sim, int64_t *out4_host);
/* verdict 1 / 0: the next nbmi_owner_step computes every wave's forces in float64 / leaves the choice to the waves;
 * -1: back to the rank's own rule. */
int nbmi_owner_set_all64(nbmi_sim *sim, int verdict);

/* Render-side reduction: NBodySimulation._compute_visibility + the gather of
 * draw() on the device (nbody/simulation.py:880-903, 927-928).  Frustum test of
 * compute_visibility_points (:403-434; z < 0.1 or z > far_dist hidden, 20 % margin) on the float64
 * device positions, then positions[mask].astype(float32) and colors[mask] (colours of the last
 * nbmi_compute_colors) in the caller's body order.  cam12 = {cam_pos, cam_forward, cam_right,
 * cam_up}.  *count = visible bodies; at most `capacity` rows are copied out.  Only the visible
 * part crosses PCIe. */
int nbmi_visible_points(nbmi_sim *sim, const double *cam12, double tan_h, double tan_v, double far_dist,
                        float *out_positions_xyz, float *out_colors_rgb, int64_t capacity, int64_t *count);
/* nbmi_export_shard / nbmi_import_ranks and the nbmi_owner_* calls synchronise the handle's stream by default.
 * With sync = 0 they only enqueue (except where a call returns counts to the host): for callers that issue
 * their collective ON the handle's stream (nbmi_stream; e.g. torch.cuda.ExternalStream). */
int nbmi_set_exchange_sync(nbmi_sim *sim, int sync);

/* Arithmetic of the Barnes-Hut pair forces (the accepted (body, node) sets are the reference's in every mode):
 *   0  per wave of 64 key-adjacent bodies: float64 where G rho dt^2 of the wave's densest quarter (16 bodies: sum of
 *      G m over the volume of their bounding box, every edge at least one softening length) exceeds `tau`
 *      (default 5e-5; tau = 0 keeps the current value), fp32 elsewhere - and float64 for EVERY wave while most of
 *      the system qualifies (entered when more than a third of a step's waves do, left below a quarter).  Default.  The reference computes in float64 throughout
 *      (nbody/simulation.py:246-268); in the dense part of a system fp32's systematic roundings are amplified to
 *      > 1e-4 of the largest coordinate within 100 steps, and where most of the system is that dense the rest
 *      follows.
 *   1  fp32 everywhere (float64 sums): fastest.
 *   2  float64 everywhere: follows the reference to ~1e-13 over 100 steps at 1 M bodies.
 * Every mode holds at softening 0 and at softenings so small that the fp32 self-term G m eps^-3 overflows: there the
 * walk skips the pairs whose dist_sq does not exceed eps^2 (the reference's rule for its own leaf and for coincident
 * bodies), in fp32 and in float64 alike.
 * Environment NBMI_FORCE_PREC / NBMI_PREC_TAU set the initial values.
 *
 * Mode 0 exactly (tests/prec_ref.py restates it, tests/test_gpu_prec_auto.py compares the device with it).  With the
 * bodies in sort-key order (rank r = 0 .. n-1), for a step of size dt:
 *   p32      = (float)x per coordinate;  g32 = (float)(G * m), the product formed in float64.
 *   group g  = the ranks [16g, 16g+16) within [0, n), aligned to the rank index;
 *   wave w   = the ranks [64w, 64w+64), that is groups 4w .. 4w+3.
 *   gsum     = the fp32 sum of the group's g32, absent ranks counting 0, associated ((w0+w1)+(w2+w3)) per four
 *              consecutive ranks, then (q0+q1)+(q2+q3) over the four quads.
 *   edge_a   = fmaxf(max p32_a - min p32_a, (float)softening) per axis, the difference taken in fp32.
 *   vol      = (edge_x * edge_y) * edge_z.
 *   dens     = gsum > 0 ? gsum / vol : 0 - vol == 0 with mass gives +inf; a group without mass or without bodies 0.
 *   D_w      = the largest dens of the wave's four groups.
 *   flag_w   = D_w > (float)(tau / dt^2)   (a threshold that overflows to +inf flags nothing: inf > inf is false).
 *   share    = (number of set flags) / ceil(n / 64).
 *   all64    = all64_rule(previous all64, ask = number of set flags, waves = ceil(n / 64), 333, 250): entered at
 *              1000 ask > 333 waves, kept while 1000 ask >= 250 waves.  nbmi_create and nbmi_set_state reset the
 *              previous value to 0.  A build that is not part of a step (nbmi_build_tree, the queries, the
 *              diagnostics, nbmi_get_accelerations_f64) changes neither the flags nor all64.  The first leapfrog step
 *              after create / nbmi_set_state contains two builds of a step - the one that primes a = F(x) at the
 *              initial positions, then the one at the drifted positions - and applies the rule once for each.
 *   In an integrating walk a wave computes in float64 iff flag_w || all64; all lanes of the wave agree.
 * The flags are cleared when the handle is created: before the first step no wave asks. */
int nbmi_set_force_precision(nbmi_sim *sim, int mode, double tau);
/* Mode 0, after a step: the share of the waves whose own density asked for float64, and whether the step ran every
 * wave in float64 (the system-wide rule above: entered when more than a third asked, left below a quarter).  Before
 * the handle's first step: (0, false).  Mode 1: (0, false); mode 2: (1, true). */
int nbmi_force_precision_share(nbmi_sim *sim, double *share, int *all_float64);
/* Native HIP stream of the handle (for ordering against framework streams). */
void *nbmi_stream(nbmi_sim *sim);

/* Frame codec on the device (tools/record.py:231-326).  A recording's .zstd frame holds either
 * absolute float32 positions + colours (format 1) or int16((cur - prev) * 1000) against the previous DECODED
 * frame (format 2, :254-262, decoder :313-322; lossy, wraps beyond +-32.767 like the reference's cast).  The
 * previous decoded frame stays in HBM, the quantisation runs on the device, and a delta frame costs 12 bytes per
 * body over PCIe instead of 24; zstd itself stays on the host.
 *   nbmi_frame_keyframe      current positions (as nbmi_get_positions_f32) and colours (of the last
 *                            nbmi_compute_colors), float32 (N,3) each; they become the previous frame
 *   nbmi_frame_delta_i16     int16 (N,3) position and colour deltas against the previous decoded frame, which is
 *                            advanced to prev + int16 / 1000 (what load_frame() will reconstruct)
 *   nbmi_frame_set_previous  restore the previous decoded frame after a resume (decoded by the host codec) */
int nbmi_frame_keyframe(nbmi_sim *sim, float *out_positions_xyz, float *out_colors_rgb);
int nbmi_frame_delta_i16(nbmi_sim *sim, int16_t *out_dpos, int16_t *out_dcol);
int nbmi_frame_set_previous(nbmi_sim *sim, const float *positions_xyz, const float *colors_rgb);

/* Asynchronous frames: take a frame without stopping the simulation.
 * A handle has NBMI_FRAME_SLOTS = 2 slots.  A slot is one device buffer and one pinned host buffer (hipHostMalloc) of
 * 24 bytes per body each, plus a 64-byte header.  They are allocated by the first nbmi_frame_begin - 2 x 24 bytes per
 * body on the device and the same again pinned on the host: 2.4 GB each at 50 M bodies - together with a copy stream and
 * two events per slot, and freed by nbmi_destroy.
 *   nbmi_frame_begin    only enqueues and never waits.  On the handle's stream one kernel reads the state once and writes
 *                       the frame (a delta frame: its float32 rows, which nbmi_frame_delta_i16's kernel then quantises)
 *                       into a free slot's device buffer in the caller's body order: float32 positions (as
 *                       nbmi_get_positions_f32) and the colours nbmi_compute_colors(sim, max_speed) computes - which it
 *                       also leaves where that call leaves them, so nbmi_get_colors_f32, nbmi_visible_points and
 *                       nbmi_render_sim afterwards see these colours.  The copy stream then copies the slot to its pinned
 *                       buffer.  *slot = the slot taken.  Steps enqueued afterwards do not touch the slot: the frame is
 *                       the state at the begin.  NBMI_FRAME_KEY / NBMI_FRAME_DELTA_I16 are nbmi_frame_keyframe /
 *                       nbmi_frame_delta_i16 with the colour pass included; they and the synchronous calls all act on
 *                       the one previous decoded frame in the order of the calls.  NBMI_ERR_ARG: no free frame slot
 *                       (nothing is overwritten, nothing changes), NBMI_FRAME_DELTA_I16 without a previous frame,
 *                       owner-mode handle.  n == 0 succeeds with empty payloads.
 *   nbmi_frame_wait     waits until THAT slot's copy is complete - not for the handle's stream, so steps enqueued after
 *                       the begin keep running.  *first / *second point into the pinned slot (positions and colours, or
 *                       position deltas and colour deltas; (N,3) each) and stay valid until nbmi_frame_release; *kind =
 *                       the kind, *steps = nbmi_step_count at the begin.  Any output pointer may be NULL.  Waiting twice
 *                       is allowed.  Deferred device errors are reported as they stood at the snapshot: NBMI_ERR_CAPACITY
 *                       / NBMI_ERR_HIP with nbmi_sync's messages; they are NOT cleared (the next nbmi_sync or getter
 *                       still reports and clears them), and the slot stays taken until it is released.
 *   nbmi_frame_release  frees the slot for the next begin.
 *   nbmi_frame_pending  the slots begun and not released, oldest first, with their kinds and step counts (arrays of
 *                       NBMI_FRAME_SLOTS; any may be NULL); returns how many (>= 0), or a negative error code.  The
 *                       recorder's Ctrl-C path asks this for the reason it asks nbmi_step_count. */
#define NBMI_FRAME_F32 0        /* float32 positions + colours (N,3) each: what get_positions + get_colors return   */
#define NBMI_FRAME_KEY 1        /* the same payload, and it becomes the previous decoded frame (nbmi_frame_keyframe) */
#define NBMI_FRAME_DELTA_I16 2  /* int16 deltas against the previous decoded frame, which advances (nbmi_frame_delta_i16) */
#define NBMI_FRAME_SLOTS 2
int nbmi_frame_begin(nbmi_sim *sim, int kind, double max_speed, int *slot);
int nbmi_frame_wait(nbmi_sim *sim, int slot, const void **first, const void **second, int *kind, int64_t *steps);
int nbmi_frame_release(nbmi_sim *sim, int slot);
int nbmi_frame_pending(nbmi_sim *sim, int *slots, int *kinds, int64_t *steps);

/* Test / measurement hook for the device sort behind the octree build ("Morton-code octree build via
 * device radix sort"; it replaces np.argsort of boids/flock.py:618 as well): sorts n (key, value) pairs
 * given as HOST arrays by the low `bits` bits of the key (key_bytes 4 or 8), stable.  impl must be 0 = the
 * hand-written gfx950 radix sort of csrc/radix.hip, the product path (the rocPRIM cross-check is a library of
 * the tests' own since round 4: tests/native/rocprim_check.hip).
 * *ms_per_sort = mean device time of `repeats` sorts after one untimed run. */
int nbmi_debug_sort_pairs(int key_bytes, int64_t n, const void *keys, const uint32_t *values, void *keys_out,
                          uint32_t *values_out, int bits, int impl, int repeats, double *ms_per_sort);
/* Its keys-only twin: sorts n HOST keys by their bits [begin_bit, end_bit), stable; the bits outside the field travel
 * with their key (the octree build sorts (prefix << 24 | body index) words this way). */
int nbmi_debug_sort_keys(int key_bytes, int64_t n, const void *keys, void *keys_out, int begin_bit, int end_bit,
                         int repeats, double *ms_per_sort);
/* Either form with the configuration of the passes given: digit_bits 8 or 10, threads per 4 096-key tile 256, 512 or
 * 1024, 0 = what the sort would choose for this size (the octree build reads NBMI_SORT_DIGIT_BITS / NBMI_SORT_THREADS
 * for the same two).  values == NULL: keys only, on the bits [begin_bit, end_bit); otherwise (key, value) pairs on
 * those bits.  Anything else is refused with NBMI_ERR_ARG before a launch. */
int nbmi_debug_sort_config(int key_bytes, int64_t n, const void *keys, const uint32_t *values, void *keys_out,
                           uint32_t *values_out, int begin_bit, int end_bit, int digit_bits, int threads, int repeats,
                           double *ms_per_sort);

/* Test hooks for the balance mode of the tree walk: from 2 M bodies on (NBMI_XCD_BALANCE=2: from
 * 8 walk blocks on) XCD x walks the logical blocks [bounds[x], bounds[x + 1]) of 256 bodies, and k_xcd_bounds cuts those
 * nine bounds from the times (4 per block, shader clocks) that the previous walk's waves left.  A walk is right exactly
 * when bounds[0] = 0, bounds[8] = nb and every range holds 1 .. jmax blocks (the launch has 8 jmax workgroups).
 *
 * nbmi_debug_xcd_bounds: the product's cut kernel with the product's jmax on 4 nb HOST words, no handle (the current
 * device).  Writes the 9 bounds and jmax.  NBMI_ERR_ARG before anything is launched, outputs untouched: nb < 8 (the cut
 * rule needs at least one block per XCD), an nb whose launch of 8 jmax workgroups no int holds, a null pointer. */
int nbmi_debug_xcd_bounds(int nb, const uint32_t *wave_cycles, int32_t *bounds9, int32_t *jmax_out);
/* nbmi_debug_wave_times: waits for everything this handle has enqueued (a cut on its side stream included) and writes
 * the 9 bounds its next balanced walk will read (all -1: none made yet, that walk cuts equal eighths from zeroed
 * times), *nb_out = its walk blocks, *jmax_out, and *balanced_walks = how many walks of the handle were launched in
 * balance mode so far.  wave_cycles != NULL (HOST, count == 4 * walk blocks): first replaces the handle's table of wave
 * times by these and cuts the bounds from them, as the first balanced walk does from zeros; the next balanced walk
 * runs on exactly these bounds.  The walks themselves and a handle that never calls this are unchanged.
 * NBMI_ERR_ARG, message "nbmi_debug_wave_times: ...": a null output, direct N^2, owner-mode and sharded handles; with a
 * table also a handle with fewer than 8 walk blocks or a walk block other than 256 (no walk of theirs runs balanced) and
 * a count other than 4 * walk blocks. */
int nbmi_debug_wave_times(nbmi_sim *sim, const uint32_t *wave_cycles, int64_t count, int32_t *bounds9, int32_t *nb_out,
                          int32_t *jmax_out, int64_t *balanced_walks);

/* ---- headless point renderer (csrc/render.hip; tools/export.py) ------------------------------------------------
 * The image fixed-function GL draws for the exporter's frame: GL_POINTS with GL_POINT_SMOOTH, glBlendFunc(GL_SRC_ALPHA,
 * GL_ONE), GL_DEPTH_TEST (GL_LESS, depth writes on), GL_EXP2 fog, gluLookAt + gluPerspective.  Where GL leaves the
 * result to the implementation, one deterministic answer is fixed here; the kernels and the tests' NumPy restatement
 * (tests/render_ref.py) both follow this text.  Arithmetic is float64 in the order written, without FMA.
 *
 * params (17 doubles): eye[3], target[3], up[3], fovy (degrees, reference 75), near (0.1), far (10000),
 * point_size (in (0, 4]; reference 1.5), fog_density (>= 0; reference 0.0003, 0 = no fog), bg[3] (in [0, 1];
 * reference (0, 0, 0.02)).  Computed once per frame on the host (C library sqrt / tan):
 *   f = normalize(target - eye), s = normalize(f x up), u = s x f        normalize(a) = a / sqrt(a.a), each component
 *   cot = 1 / tan(fovy * pi / 360), aspect = W / H
 *   za = (far + near) / (near - far), zb = 2 * far * near / (near - far)  (left to right)
 * Per point, p = the float32 position converted exactly, e = p - eye (per component), a.b = (a0 b0 + a1 b1) + a2 b2:
 *   x_e = s.e, y_e = u.e, z_e = -(f.e)
 *   x_c = (cot / aspect) x_e, y_c = cot y_e, z_c = za z_e + zb, w_c = -z_e
 *   clip: the point is drawn only if |x_c| <= w_c and |y_c| <= w_c and |z_c| <= w_c (else discarded whole)
 *   x_w = (x_c / w_c)(W / 2) + W / 2, y_w = (y_c / w_c)(H / 2) + H / 2
 *   depth d = floor(((z_c / w_c) 0.5 + 0.5)(2^24 - 1) + 0.5)
 *   coverage, R = point_size / 2: pixel (i, j) with floor(x_w - R) <= i <= floor(x_w + R) (same for j), inside
 *     [0, W) x [0, H), gets c = the number of its 16 samples (i + (a + 1/2)/4, j + (b + 1/2)/4), a, b in 0..3, with
 *     dx dx + dy dy <= R R (dx = sample x - x_w, dy likewise); a fragment exists where c >= 1
 *   fog = exp(-(t t)), t = fog_density (-z_e);  C = clamp(colour, 0, 1) (NaN -> 0);
 *     C' = fog C + (1 - fog) bg;  v = floor(C' 4080 + 0.5) per channel
 * Fragments are taken in the caller's row order.  One passes iff d < 2^24 - 1 and d < the d of every earlier fragment
 * of the same pixel (GL_LESS against a depth buffer cleared to 2^24 - 1 that every fragment leaves at its minimum).
 * Per pixel and channel A = sum over passing fragments of c v (an exact integer), and the output is
 *   min(255, bg8 + ((A + 128) >> 8)),  bg8 = floor(bg 255 + 0.5)
 * as uint8 (H, W, 3) RGB with row 0 at the TOP (glReadPixels, then flipud).  Window pixel (i, j) is image row H-1-j.
 * The image depends on draw order only through the exact depth rule: it is the same bytes on every run.  Device exp
 * may differ from the C library's by an ulp, which can move a fogged v by one.
 *
 * A renderer owns one stream, its device buffers and a pinned image buffer, and is used from one host thread at a
 * time.  Sizes up to 16384 x 16384; at most 2^27 - 1 points; a frame of more than 2^30 - 1 fragments is refused
 * with NBMI_ERR_CAPACITY.  n == 0, or every point clipped, gives the background image. */
typedef struct nbmi_render nbmi_render;
/* NULL (message in nbmi_last_error) on bad size or device. */
nbmi_render *nbmi_render_create(int width, int height, int device);
void nbmi_render_destroy(nbmi_render *r);
/* Host arrays (N,3) float32, caller's row order; out_rgb = W*H*3 bytes.  Uploads go through pinned staging. */
int nbmi_render_points(nbmi_render *r, const float *positions_xyz, const float *colors_rgb, int64_t n,
                       const double *params, uint8_t *out_rgb);
/* The handle's current positions (as nbmi_get_positions_f32) and the colours of its last nbmi_compute_colors, read on
 * the device.  The handle and the renderer must be on the same device; owner-mode handles are refused. */
int nbmi_render_sim(nbmi_render *r, nbmi_sim *sim, const double *params, uint8_t *out_rgb);
/* Of the last frame: {points drawn (centre inside the clip volume), fragments, passing fragments, pixels with at
 * least one fragment}. */
int nbmi_render_stats(nbmi_render *r, int64_t *out4);
/* Device time of the last frame in ms: {project + emit, sort, resolve, pack + copy to the host}. */
int nbmi_render_timers(nbmi_render *r, double *out_ms4);

#ifdef __cplusplus
}
#endif
#endif /* NBMI_H */
