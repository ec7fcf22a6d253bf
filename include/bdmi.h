/*
 * bdmi.h - C ABI of the MI355X-native boids neighbour sweep (part of libnbmi.so).
 *
 * The reference has no backend seam for boids; its operator boundary is the five flat-array
 * @njit kernels driven by Flock.update (reference boids/flock.py:627-678):
 *   assign_cells              boids/flock.py:30-44   (get_cell_index :16-27)
 *   np.argsort + build_cell_lists   boids/flock.py:610-625, :47-65
 *   compute_flocking_spatial  boids/flock.py:68-238
 *   update_physics_numba      boids/flock.py:241-308
 * bdmi_step() is one Flock.update(dt): all four stages on the device, float64 state and
 * arithmetic as in the reference, state resident in HBM between steps.
 * Arrays crossing the boundary are C-order (N,3) float64, rows in the caller's boid order.
 * Return codes / error string as in nbmi.h (bdmi_last_error == nbmi_last_error).
 */
#ifndef BDMI_H
#define BDMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct bdmi_flock bdmi_flock;

/* params[11] in the order of reference config/boids.py:30-46:
 * bounds, wall_margin, wall_weight, max_speed, max_force, perception_radius,
 * separation_radius, separation_weight, alignment_weight, cohesion_weight, color_blend_rate.
 * Grid as Flock.__init__ (flock.py:478-481): cell = perception_radius,
 * dim = ceil(2*bounds/cell) + 2, offset = bounds + cell. */
bdmi_flock *bdmi_create(int64_t n, const double *positions_xyz, const double *velocities_xyz,
                        const double *colors_rgb, const double *params11, int device);
void bdmi_destroy(bdmi_flock *f);
const char *bdmi_last_error(void);

/* `substeps` x Flock.update(dt) (flock.py:627-678), enqueued without host synchronisation. */
int bdmi_step(bdmi_flock *f, double dt, int substeps);
int bdmi_sync(bdmi_flock *f);

/* positions / velocities / colors (N,3) float64 each; any pointer may be NULL. */
int bdmi_get_state(bdmi_flock *f, double *positions_xyz, double *velocities_xyz, double *colors_rgb);
int bdmi_set_state(bdmi_flock *f, const double *positions_xyz, const double *velocities_xyz,
                   const double *colors_rgb);

/* ---- parity hooks ------------------------------------------------------------------- */
/* assign_cells output for the current positions: (N,) int32, caller's boid order. */
int bdmi_get_cell_indices(bdmi_flock *f, int32_t *cell_indices);
/* compute_flocking_spatial outputs for the current state (no physics applied):
 * separation / alignment / cohesion forces and avg_colors, (N,3) float64 each, with the
 * caller-side pre-fill of Flock.update (forces 0, avg_colors = colors; flock.py:633-636). */
int bdmi_get_forces(bdmi_flock *f, double *sep, double *ali, double *coh, double *avg_colors);
/* grid facts: dim, num_cells, non-empty cells of the last built grid.  The last built grid is that of the last
 * bdmi_step, or of the current positions after bdmi_get_forces, one of the four flock-analysis calls (or their three
 * periodic counterparts), bdmi_topological_neighbours or bdmi_velocity_correlation (with nb > 0) below. */
int bdmi_grid_info(bdmi_flock *f, int32_t *grid_dim, int64_t *num_cells, int64_t *occupied);
/* device ms accumulated per phase [cells+sort, reorder+table, sweep+physics], steps counted */
int bdmi_enable_timers(bdmi_flock *f, int enable);
int bdmi_get_timers(bdmi_flock *f, double *ms3, int64_t *count, int reset);


/* ---- flock analysis: flock finder, catalogue, order parameters, neighbour statistics ----------
 * The boids counterpart of nbmi_diagnostics + nbmi_fof + nbmi_fof_catalogue, on the sweep's own grid.  This text is the
 * specification; the kernels (csrc/bdmi.hip) and the tests' NumPy restatement (tests/flockstats_ref.py) both follow it.
 * Arithmetic is float64 in the association written, without FMA; sqrt and divide are correctly rounded.
 *
 * For the handle's current state:
 *   d2(i, j) = (dx dx + dy dy) + dz dz with dx = x_j - x_i (k_flock's association; symmetric in i and j).
 *   b2 = link * link, one float64 product computed on the host.  `link` (and `radius` below) must be finite, > 0 and
 *     <= perception_radius: the grid cell is the perception radius, so the 27-cell neighbourhood covers it.
 *   Boids i != j are LINKED iff d2(i, j) <= b2.  Equality links and a coincident pair is linked: nbmi_fof's rule.  This
 *     is deliberately NOT the sweep's window 1e-4 < d2 < r^2 (flock.py:148): a clustering that splits coincident boids
 *     is useless.
 *   A FLOCK is a connected component of the link graph; a boid without a friend is a flock of one.
 *   Boids outside the grid are clamped into its border cells as in get_cell_index (flock.py:16-27).  Clamping is monotone
 *     per axis, so two linked boids (at most one cell apart per axis before clamping) are still in the same or in
 *     adjacent cells: every result below stays exact there.
 *
 * bdmi_flocks: labels[i] (caller's boid order) = the smallest caller index in i's flock: unique, independent of the
 *   evaluation order, equal to a brute force's.  *n_flocks = the number of distinct labels.  *links = the exact number of
 *   unordered linked pairs: every candidate pair is evaluated exactly once, and a pair is not skipped because its boids
 *   are in one set already.  *evals = the number of d2 evaluated (a measurement hook like nbmi_fof's).
 * bdmi_flock_catalogue: the flocks with members >= min_members (min_members >= 1), ordered by members descending, ties
 *   by label ascending.  *count = the number of qualifying flocks, which may exceed `capacity`; at most `capacity` rows
 *   are copied out, the first ones of that order (as nbmi_fof_catalogue).  label / members / rows16 may be NULL when
 *   capacity == 0.
 * The ROW of 16 doubles, of one flock here and of the whole flock in bdmi_diagnostics (every boid in one group, no link
 *   evaluated):  {m, c[3], vbar[3], polarisation, mean_speed, milling, lo[3], hi[3]}.  For the group's members j = 1..m:
 *     s_j = sqrt((vx vx + vy vy) + vz vz);  u_j = v_j / s_j per component, 0 when s_j == 0
 *     Sp = sum p_j, Sv = sum v_j, Su = sum u_j, Ss = sum s_j
 *     c = Sp / m, vbar = Sv / m, mean_speed = Ss / m
 *     polarisation = sqrt((Su_x^2 + Su_y^2) + Su_z^2) / m        (1: perfectly aligned; about m^-1/2: disordered)
 *   second pass, with r_j = p_j - c (the rounded c):
 *     rho_j = sqrt((rx rx + ry ry) + rz rz);  rhat_j = r_j / rho_j per component, 0 when rho_j == 0
 *     w_j = rhat_j x u_j = (ry uz - rz uy, rz ux - rx uz, rx uy - ry ux)
 *     milling = sqrt((Wx^2 + Wy^2) + Wz^2) / m with W = sum w_j  (the rotational order parameter)
 *   lo / hi = the exact per-axis minimum / maximum of the positions.
 *   The sums are float64 in an order fixed for a given state, without floating-point atomics: two calls on an unchanged
 *   state return the same bits.  Members are taken in the order a stable sort by label leaves the cell-sorted boids, cut
 *   into chunks of 4096 consecutive members; one block reduces a chunk with a fixed tree and the chunks' partials are
 *   added in chunk order, so a flock of all N boids is N / 4096 blocks and not one wave's loop.  bdmi_diagnostics uses
 *   the same chunk reduction over the cell-sorted boids, without the sort by label: where one flock covers all boids its
 *   catalogue row and the bdmi_diagnostics row are the same bits.  N == 0: m = 0 and the rest zeros.
 * bdmi_neighbour_stats: count[i] = #{j != i : d2(i, j) <= radius^2}, nn_d2[i] = the smallest such d2, +inf when
 *   count[i] == 0.  Exact and order independent; the sum of count is 2 * links of bdmi_flocks at link == radius.
 *
 * All four build the grid for the current positions (as bdmi_get_forces does; bdmi_grid_info's `occupied` then describes
 * that grid), change nothing a later step reads - a run with calls between its steps gives the same state bits as one
 * without - wait for their own work and report the sort's sticky error like bdmi_sync.  N == 0: success, zeros,
 * *count = 0; N == 1: one flock of one.  Refused with NBMI_ERR_ARG (message "<call>: ..."), before anything is launched
 * and with the outputs untouched: a link or radius that is not finite, <= 0 or above the perception radius (the message
 * names both numbers), min_members < 1, capacity < 0, and slab handles (bdmi_create_slab).
 * Scratch, allocated at the first of these calls and freed by bdmi_destroy: 52 bytes per boid (union-find parent, root,
 * least id and members per root, members per label, labels and ranks unsorted and sorted, two key / value pairs for
 * the catalogue's heads); per catalogue row copied out 144 bytes plus 128 bytes per chunk of 4096 members.  The labels
 * and neighbour statistics travel through the state staging buffer. */
int bdmi_flocks(bdmi_flock *f, double link, int32_t *labels /* (N,), may be NULL */, int64_t *n_flocks,
                int64_t *links, int64_t *evals); /* each may be NULL */
int bdmi_flock_catalogue(bdmi_flock *f, double link, int64_t min_members, int64_t capacity, int32_t *label,
                         int64_t *members, double *rows16, int64_t *count);
int bdmi_diagnostics(bdmi_flock *f, double *row16);
int bdmi_neighbour_stats(bdmi_flock *f, double radius, int32_t *count /* (N,) */, double *nn_d2 /* (N,) */,
                         int64_t *evals); /* each output may be NULL */

/* ---- topological interaction: the k nearest neighbours within sight ----------------------------
 * The reference knows one interaction rule, the metric one: every boid within perception_radius counts.  The other
 * standard flocking model is topological (Ballerini et al. 2008: starlings interact with their 6-7 nearest neighbours,
 * whatever their distance), which gives flocks whose cohesion does not depend on their density.  It is opt-in per handle:
 * a handle that never enables it runs the metric kernels and gives their bits.  This text is the specification; the
 * kernel (csrc/bdmi.hip, k_flock_topo) and the tests' NumPy restatement (tests/topo_ref.py) both follow it.
 *
 * For the handle's current state and a boid i:
 *   d2(i, j) = (dx dx + dy dy) + dz dz with dx = p_i - p_j, float64, no FMA: the sweep's own expression.
 *   The METRIC set N_i = { j != i : 1e-4 < d2(i, j) < perception_radius^2 }: exactly the reference's window (flock.py:150).
 *   The TOPOLOGICAL set T_i = the min(k, |N_i|) members of N_i that come first in ascending lexicographic order of
 *     (d2(i, j), id_j), id_j being the caller's boid index.  The tie-break makes T_i unique.
 *   STILL BOUNDED BY PERCEPTION: a neighbour is never further away than the perception radius.  This is "the k nearest
 *     within sight", not an unbounded k-nearest search: the 27-cell neighbourhood of the sweep's grid covers it exactly.
 *   Forces and colours: compute_flocking_spatial's formulas (flock.py:150-238) with T_i in the place of the neighbour
 *     set: neighbor_count = |T_i|; the separation terms come from those members of T_i with d2 < separation_radius^2;
 *     avg_colors = (sum over T_i + own) / (|T_i| + 1); steer(), the pre-fill and update_physics_numba are unchanged.
 *   FIXED SUMMATION ORDER: every per-boid sum (separation, alignment, cohesion, colour) starts at +0.0 and adds its terms
 *     one by one in the order of T_i above.  With correctly rounded sqrt and divide and without FMA, the four force arrays
 *     and the stepped state are a pure function of the state and the ids: they do not depend on the cell order, on what
 *     earlier steps did to the row order, or on the block order (BDMI_XCD), and a NumPy restatement reproduces them bit
 *     for bit, separation included (the metric sweep's separation sum has no such order).
 *   1 <= k <= 16.
 *
 * bdmi_set_neighbour_mode: BDMI_NEIGHBOURS_METRIC (the default: the reference's rule, the metric kernels; k is ignored and
 *   the handle's k is kept) or BDMI_NEIGHBOURS_TOPOLOGICAL with k.  bdmi_step and bdmi_get_forces follow the handle's mode;
 *   the topological sweep counts in phase 3 of the timers.  bdmi_get_neighbour_mode reads the mode and k back.
 * bdmi_topological_neighbours: a parity hook like bdmi_get_cell_indices, in either mode and with its own k.  Row i
 *   (caller's order) of ids / d2 lists T_i's ids in order and their d2, padded with -1 / +inf; count[i] = |T_i|.  It
 *   builds the grid for the current positions as bdmi_get_forces does and changes nothing a later step reads.
 * Refused with NBMI_ERR_ARG (message "<call>: ..."), before anything is launched and with the outputs and the mode
 *   untouched: an unknown mode, k outside 1..16 (the message names k), a null handle, and slab handles
 *   (bdmi_create_slab) for both the setter and the hook.  Slab support is a follow-up: the order (d2, GLOBAL id) would
 *   make the slabs' results bit-identical to one GPU's, since nothing else of a slab's row order enters the sums.
 * N == 0 and N == 1 succeed: zero forces, count = 0.
 * Environment BDMI_NEIGHBOURS, read at create like BDMI_XCD: "topological" or "topological:K" (K in 1..16, default 7) sets
 *   the initial mode of handles that allow it; anything else means metric.  It lets unchanged drivers run in this mode.
 * Scratch of the hook, allocated at its first call: 12 k + 4 bytes per boid. */
#define BDMI_NEIGHBOURS_METRIC 0
#define BDMI_NEIGHBOURS_TOPOLOGICAL 1
int bdmi_set_neighbour_mode(bdmi_flock *f, int mode, int k);
int bdmi_get_neighbour_mode(bdmi_flock *f, int *mode, int *k); /* either may be NULL */
int bdmi_topological_neighbours(bdmi_flock *f, int k, int32_t *ids /* (N,k) */, double *d2 /* (N,k) */,
                                int32_t *count /* (N,) */); /* each may be NULL */

/* ---- periodic box and seeded vectorial noise ----------------------------------------------------
 * The experiment the order parameters of bdmi_diagnostics exist for - order against noise (Vicsek et al. 1995; Gregoire &
 * Chate 2004; Ballerini et al. 2008 for the topological rule) - needs a domain without walls and a noise amplitude to
 * sweep.  Both are opt-in: a handle made by bdmi_create that never sets noise runs the kernels it ran before and gives
 * their bits.  This text is the specification; the kernels (csrc/bdmi.hip) and the tests' NumPy restatements
 * (tests/periodic_ref.py, tests/noise_ref.py) both follow it.  All arithmetic is float64 in the association written,
 * without FMA, with correctly rounded sqrt and divide.
 *
 * PERIODIC HANDLES: bdmi_create_periodic, same arguments as bdmi_create.
 *   Box and grid: B = bounds, L = 2 * B (one float64 product); the box is [-B, B] per axis.  dim = floor(L /
 *     perception_radius), cell_size = L / dim (so cell_size >= perception_radius), offset = B.  The cell coordinate of x is
 *     int((x + offset) / cell_size) clamped to [0, dim - 1], so x == +B falls into the last cell.
 *   Refused with NBMI_ERR_ARG: dim < 3 or dim > 1290 (with dim < 3 the 27 wrapped cells are not distinct, and a neighbour
 *     has more than one image in sight); at create and at bdmi_set_state a position that is not finite or outside [-B, B]:
 *     the message names the first offending row and nothing is uploaded.  wall_margin and wall_weight are ignored
 *     (wall_margin > 0 is not required).
 *   The IMAGE of a candidate j for boid i, per axis: d0 = p_i - q_j; q' = q_j + L if d0 > B, q' = q_j - L if d0 < -B,
 *     otherwise q' = q_j.  Equality does not shift.  From here on q' stands in for the neighbour's position in every
 *     formula of compute_flocking_spatial: dx = p_i - q', d2 = (dx dx + dy dy) + dz dz, the window 1e-4 < d2 <
 *     perception_radius^2 is unchanged, the separation terms come from dx, the cohesion sum adds q'.  Where no shift
 *     happens the operations and the bits are those of a walled handle.
 *   The candidate cells are the 27 cells (cx+a, cy+b, cz+c) mod dim.  With dim >= 3 and cell_size >= perception_radius
 *     each boid is a candidate exactly once, and its image above is the only one that can be in the window.
 *   Both neighbour modes work.  In topological mode the order is (d2, id) with the d2 above and the fixed summation order
 *     holds, so forces and stepped state are a pure function of state and ids.
 *   Physics: update_physics_numba without the wall terms.  After p' = p + v' dt, per axis: if p' > B then p' = p' - L,
 *     else if p' < -B then p' = p' + L.  bdmi_step on a periodic handle requires max_speed * |dt| < L (-1 otherwise and
 *     nothing is run, like the slab rule): one wrap is then enough and the state stays inside [-B, B].
 *   bdmi_get_box: each output may be NULL.  Walled handles give periodic = 0, length = 2 * bounds, cell_size =
 *     perception_radius; periodic ones 1, L and L / dim.
 *   Work unchanged on periodic handles: bdmi_get_state, bdmi_set_state, bdmi_get_cell_indices (the periodic grid's
 *     indices), bdmi_get_forces, bdmi_topological_neighbours (d2 is the image d2), bdmi_set_neighbour_mode /
 *     bdmi_get_neighbour_mode, BDMI_NEIGHBOURS, bdmi_grid_info, the timers, bdmi_visible_vertices, bdmi_render_flock, and
 *     bdmi_diagnostics: polarisation, mean speed and vbar do not depend on positions; c, milling, lo and hi are computed
 *     from the coordinates in the box as they stand (a flock that straddles a face has its centre in between).
 *   Refused on periodic handles with NBMI_ERR_ARG ("<call>: ... periodic ..."), before anything is launched and with the
 *     outputs untouched: bdmi_flocks, bdmi_flock_catalogue, bdmi_neighbour_stats.  Their counterparts through the faces
 *     are bdmi_periodic_flocks, bdmi_periodic_flock_catalogue and bdmi_periodic_neighbour_stats ("Flock analysis on
 *     periodic handles" below).  There is no periodic slab handle.
 *
 * NOISE, on walled and periodic handles, not on slab handles.
 *   bdmi_set_noise(f, eta, seed, step): eta must be finite and >= 0.  step >= 0 sets the handle's noise step, step == -1
 *     keeps it.  bdmi_get_noise reads all three back; each output may be NULL.
 *   The noise step of a handle starts at 0 at create and advances by one per Flock.update, that is per substep of
 *     bdmi_step, whether or not eta > 0.  bdmi_set_state does not touch it.
 *   The unit vector xi_i(step) of the boid with caller id i.  For attempts a = 0, 1, 2, ...: the Philox4x32-10 block with
 *     counter {i, (uint32)step, (uint32)(step >> 32), a} and key {(uint32)seed, (uint32)(seed >> 32)} yields words
 *     w0..w3; pair 0 is (w0, w1), pair 1 is (w2, w3).  For a pair (u, v): x1 = ((double)u + 0.5) * 2^-31 - 1, x2 likewise
 *     from v, s = x1 x1 + x2 x2.  The first pair with s < 1 is accepted (pair 0 before pair 1, attempt a before a + 1).
 *     Then t = sqrt(1 - s) and xi = ((2 x1) t, (2 x2) t, 1 - 2 s): Marsaglia 1972, correctly rounded operations only.
 *   How it enters the step: A = eta * max_force is one host product; acc_c = ((sep_c + ali_c) + coh_c) + A * xi_c; the
 *     wall terms of a walled handle follow, then the unchanged velocity clamp and integration.  The four arrays of
 *     bdmi_get_forces do not contain the noise.  With eta == 0 the step's operations are exactly those without noise: no
 *     "+ 0.0 * xi".
 *   bdmi_noise_vectors(f, step, out): a parity hook: xi_i(step) under the handle's seed, rows in the caller's order, for
 *     any step >= 0; step == -1 means the handle's current step.  It works with eta == 0 and changes nothing a later step
 *     reads.
 *   Refused with NBMI_ERR_ARG ("<call>: ..."), outputs and settings untouched: a null handle, a slab handle (for
 *     bdmi_get_box too), an eta that is negative or not finite (the message names it), step < -1. */
bdmi_flock *bdmi_create_periodic(int64_t n, const double *positions_xyz, const double *velocities_xyz,
                                 const double *colors_rgb, const double *params11, int device);
int bdmi_get_box(bdmi_flock *f, int *periodic, double *length, double *cell_size); /* each may be NULL */
int bdmi_set_noise(bdmi_flock *f, double eta, uint64_t seed, int64_t step);
int bdmi_get_noise(bdmi_flock *f, double *eta, uint64_t *seed, int64_t *step); /* each may be NULL */
int bdmi_noise_vectors(bdmi_flock *f, int64_t step, double *out_xyz /* (N,3) */);

/* ---- flock analysis on periodic handles: flocks, catalogue and neighbour counts through the faces
 * bdmi_flocks, bdmi_flock_catalogue and bdmi_neighbour_stats on the periodic box of bdmi_create_periodic, under names of
 * their own: the walled calls keep refusing a periodic handle, and these three refuse a walled one.  This text is the
 * specification; the kernels (csrc/bdmi.hip) and the tests' NumPy restatement (tests/torus_ref.py) both follow it.
 * Arithmetic is float64 in the association written, without FMA; sqrt and divide are correctly rounded.  B, L, dim,
 * cell_size and the cell coordinate are those of "Periodic handles" above.
 *
 * DISTANCE.  Per axis dx = x_j - x_i; if dx > B then dx = dx - L, else if dx < -B then dx = dx + L.  Equality does not
 *   shift.  d2(i, j) = (dx dx + dy dy) + dz dz.  The rule acts on the DIFFERENCE, not on the neighbour's position as the
 *   sweep's image does: x_i - x_j is exactly -(x_j - x_i) and both shifts are mirror images, so d2(i, j) and d2(j, i) are
 *   the same bits and the link relation is symmetric whichever boid of a pair evaluates it.  The sweep's image-of-position
 *   rule does not guarantee that: for a pair through a face this d2 may differ in the last bit from the d2 of
 *   bdmi_topological_neighbours.
 * LINKS.  As in the flock analysis above: b2 = link * link (one host product), boids i != j are linked iff d2(i, j) <= b2,
 *   equality links, a coincident pair is linked.  `link` (and `radius`) must be finite, > 0 and <= perception_radius.  The
 *   candidates of a boid are the 27 cells (cx+a, cy+b, cz+c) mod dim; with dim >= 3 and cell_size >= perception_radius
 *   they are distinct and cover the link, so every pair is evaluated exactly once.
 * bdmi_periodic_flocks: labels, *n_flocks, *links and *evals mean what they mean in bdmi_flocks.
 * bdmi_periodic_neighbour_stats: as bdmi_neighbour_stats with this d2; the sum of count is 2 * links at link == radius.
 * bdmi_periodic_flock_catalogue: selection, order, *count, capacity and the member order as in bdmi_flock_catalogue.  The
 *   ROW of a flock on the torus:
 *     cc_a(j) = the cell coordinate of member j on axis a (the decomposition of bdmi_get_cell_indices: index = cc_x +
 *       cc_y dim + cc_z dim^2);  O_a = the set of cell coordinates the flock's members occupy on axis a.
 *     The flock SPANS axis a if |O_a| == dim: wrap_a = -1 and the coordinates on that axis are taken as they stand,
 *       y_ja = x_ja.  Spanning is necessary for a flock that winds around the box, not sufficient: a C-shaped flock that
 *       has a member in every slab without closing also spans.
 *     Otherwise wrap_a = s_a, the smallest c in O_a whose cyclic predecessor (c - 1 + dim) mod dim is not in O_a (one
 *       exists), and y_ja = x_ja + L if cc_a(j) < s_a, else x_ja: one float64 add.  With link <= cell_size no link crosses
 *       an empty slab, so the occupied slabs of a connected flock form one cyclic arc and this cut is the geometrically
 *       right one; the rule is the definition whatever the geometry.
 *     The 16 doubles have the layout and formulas of the row above with y in the place of p:  Sp = sum y_j, c~ = Sp / m;
 *       the row's c_a = c~_a - L if c~_a > B, else c~_a;  lo / hi = the exact minimum / maximum of y (hi may exceed B;
 *       hi - lo is the flock's extent);  the second pass uses r_j = y_j - c~, the unwrapped centre before it is brought
 *       back;  vbar, polarisation and mean_speed do not see positions and are unchanged.
 *     Member order, the chunks of 4096, the fold inside a chunk and the chunk order are exactly those of the row above, on
 *       the periodic grid's cell order: two calls on an unchanged state give the same bits.
 *   wrap3 (capacity, 3) int32, may be NULL: wrap_a of every row copied out.
 * Unchanged from the walled calls: N == 0 (success, zeros, *count = 0) and N == 1 (one flock of one, whose wrap_a is its cell
 *   coordinate); "changes nothing a later step reads"; the sort's sticky error; bdmi_grid_info
 *   afterwards describes the grid of the current positions.
 * Refused with NBMI_ERR_ARG (message "<call>: ..."), before anything is launched and with the outputs untouched: a walled
 *   handle (the message names the walled call to use), a slab handle, a null handle, a link or radius that is not finite,
 *   <= 0 or above the perception radius (the message names both numbers), min_members < 1, capacity < 0, a null count, or
 *   a null label / members / rows16 with capacity > 0.
 * Scratch on top of the flock analysis': per catalogue row copied out 12 * ceil(dim / 32) bytes of occupancy words, 24 bytes
 *   of unwrapped centre and 12 bytes of wrap3. */
int bdmi_periodic_flocks(bdmi_flock *f, double link, int32_t *labels /* (N,), may be NULL */, int64_t *n_flocks,
                         int64_t *links, int64_t *evals); /* each may be NULL */
int bdmi_periodic_flock_catalogue(bdmi_flock *f, double link, int64_t min_members, int64_t capacity, int32_t *label,
                                  int64_t *members, double *rows16, int32_t *wrap3 /* (capacity,3), may be NULL */,
                                  int64_t *count);
int bdmi_periodic_neighbour_stats(bdmi_flock *f, double radius, int32_t *count /* (N,) */, double *nn_d2 /* (N,) */,
                                  int64_t *evals); /* each output may be NULL */

/* ---- velocity correlation C(r) beyond the sight radius ------------------------------------------
 * The connected correlation of the heading fluctuations as a function of distance (Cavagna et al. 2010; the finite-size
 * susceptibility of Attanasi et al. 2014 comes from the same sums), and with the same counts the radial distribution.  The
 * boids counterpart of nbmi_pair_counts, and the one boids call that looks further than one cell.  It works on walled and
 * periodic handles under one name.  This text is the specification; the kernels (csrc/bdmi.hip) and the tests' NumPy
 * restatement (tests/vcorr_ref.py) both follow it.  Every result is a set of integers: unique, independent of the caller
 * order, the cell order and the block order, equal to a brute force's.
 *
 * HEADINGS.  s_i and u_i are the row's above: s = sqrt((vx vx + vy vy) + vz vz), u_c = v_c / s, 0 when s == 0; float64
 *   without FMA.
 * FLUCTUATION AND QUANTISATION.  mean3 is required, finite, |mean_c| <= 1.  d_c = u_ic - mean_c (one float64 subtraction);
 *   q_ic = rint(d_c 2^24), ties to even, as an integer (the product by a power of two is exact); q_ic = 0 where d_c is not
 *   finite.  So |q_ic| <= 2^25, and a pair's g_ij = q_ix q_jx + q_iy q_jy + q_iz q_jz is an exact integer, |g_ij| <= 3 * 2^50.
 *   The quantum 2^-24 is part of the specification: 6e-8 of a unit heading, far below any fluctuation of interest, and what
 *   makes every sum below an integer.
 * EDGES, as nbmi_pair_counts': nb + 1 float64 values, 1 <= nb <= 64, finite, edges[0] >= 0, strictly increasing;
 *   E[k] = edges[k] * edges[k] (one host product each) must again be finite and strictly increasing.  Slot 0 of pairs and
 *   dot is "below": the pairs with d2 <= E[0].  Slot k >= 1 holds those with E[k-1] < d2 <= E[k]: the upper edge belongs
 *   to the bin.  A pair with d2 > E[nb] (or a d2 that is NaN) is in no slot.
 * DISTANCE.  d2(i, j) is fs_d2 of the flock analysis on a walled handle and the difference-based minimum image of "Flock
 *   analysis on periodic handles" on a periodic one: the same bits from either boid of a pair.
 * REACH AND THE CANDIDATE RULE.  m = (int)ceil(edges[nb] / cell_size), one float64 divide, cell_size that of bdmi_get_box.
 *   Required: 1 <= m <= 16, and on a periodic handle 2 m + 1 <= dim: then the (2m+1)^3 wrapped cells are distinct and
 *   edges[nb] <= m cell_size < B, so the minimum image is the only one in range.
 *   A pair {i, j}, i != j, is a CANDIDATE iff on every axis its cell coordinates (those of bdmi_get_cell_indices) differ by
 *   at most m: the clamped coordinates on a walled handle, the cyclic difference min(|D|, dim - |D|) on a periodic one.
 *   The candidate rule is the definition, as the catalogue's cut rule is.  Every candidate pair is evaluated exactly once;
 *   *evals = their number.  A pair whose exact separation is below edges[nb] is always a candidate, except possibly within
 *   a rounding of m cell_size (the cell coordinate is a rounded quotient).  Clamping is monotone, so boids outside a
 *   walled grid stay exact.
 * OUTPUTS.  pairs[k] = the number of candidate pairs in slot k.  dot[2k], dot[2k+1] = (hi, lo) of S_k = the sum of g_ij over
 *   those pairs: S_k = hi 2^32 + lo with 0 <= lo < 2^32, which makes (hi, lo) unique; |S_k| can pass 2^63.  The device
 *   carries three 64-bit integer words per slot with explicit carries, exact while |S_k| < 2^95, the range of (hi, lo)
 *   itself: at the largest |g_ij| that is 2^43 pairs in one slot.
 *   self5 = {sum q_ix, sum q_iy, sum q_iz, Q_hi, Q_lo} with Q = sum (q_ix^2 + q_iy^2 + q_iz^2) in the same form, over all
 *   boids, without the grid (N 2^25 < 2^56: the three sums fit).  With a last edge that reaches every pair,
 *   2 sum_k S_k == |sum q|^2 - Q.
 *   nb == 0 is allowed (edges may then be NULL): only self5 is computed, no grid is built, *evals = 0, pairs and dot are
 *   not written.  With mean3 = 0 this is the exact integer heading sum.
 * It builds the grid for the current positions as bdmi_get_forces does (bdmi_grid_info then describes that grid), changes
 *   nothing a later step reads, waits for its own work and reports the sort's sticky error.  N == 0 and N == 1 succeed
 *   with zeros (self5 of the one boid).
 * Refused with NBMI_ERR_ARG (message "bdmi_velocity_correlation: ..."), before anything is launched and with the outputs
 *   untouched: a null handle, a slab handle, nb outside 0..64, null edges with nb > 0, null mean3, a bad edge (the message
 *   names its index and value), m outside its range (the message names m, dim and the largest admissible last edge), a
 *   mean3 that is not finite or above 1 in magnitude.
 * Scratch, allocated at the first call and freed by bdmi_destroy: 16 bytes per boid (q as int4, the caller id in the
 *   fourth word) and 2 184 bytes of counters and edges. */
int bdmi_velocity_correlation(bdmi_flock *f, int nb, const double *edges /* nb+1 */, const double *mean3,
                              int64_t *pairs /* nb+1 */, int64_t *dot /* (nb+1, 2): hi, lo */, int64_t *self5,
                              int64_t *evals); /* each output may be NULL */

/* ---- multi-GPU: x-slabs with a one-cell halo -----------------------------------------
 * A rank owns the boids with x_lo <= x < x_hi (a whole number of cell planes, at least two cells wide); the
 * neighbour sweep needs the boids within one cell (= the perception radius, flock.py:479) on the other side
 * of each face.  The handle holds the owned boids plus this step's ghosts (read-only copies of the
 * neighbours' boundary boids).  The speed clamp bounds a step's displacement by max_speed * |dt|, and a handle knows
 * of its neighbours only that they are at least two cells wide, so bdmi_step on a slab handle REQUIRES
 * max_speed * |dt| < 2 * perception_radius (-1 otherwise, nothing is run): then a boid that leaves its slab lands
 * inside the adjacent one, and ONE exchange per step carries migrants and halo alike.  (Beyond that a boid could land
 * in a slab that never received it, and no rank would own it after the next export.  The halo does not depend on
 * the step: it is taken from the positions at the start of the step.  Ordinary handles are not limited.)
 *
 *   bdmi_slab_export(h, left, &nl, right, &nr)   drop last step's ghosts; rows {p, v, c, global id} (10 doubles)
 *                                                of the owned boids with x < x_lo + cell -> `left`, with
 *                                                x >= x_hi - cell -> `right` (device buffers, counts on the
 *                                                host); owned boids now outside the slab stay as ghosts
 *        exchange with the two neighbours        (send/recv or all-to-all-v on the host framework)
 *   bdmi_slab_import(h, rows, count)             received rows: inside the slab -> owned, else ghosts
 *   bdmi_step(h, dt, 1)                          Flock.update for the owned boids; ghosts only take part as
 *                                                neighbours
 *
 * The candidate set of every owned boid equals the single-GPU one, so forces agree to float64 summation
 * order.  bdmi_slab_get returns the owned rows (10 doubles each, any order): at most `capacity` rows are copied,
 * *count is the full number.  bdmi_slab_import beyond the handle's capacity returns -4 and changes nothing.
 * bdmi_slab_count compacts the handle to its owned rows (this step's ghosts are dropped) and returns their number.
 *
 * A slab handle keeps GLOBAL ids (and -1 - id for a ghost), a part of the flock, and a row count that changes with
 * every exchange, so the calls that address caller-order arrays by id - bdmi_get_state, bdmi_set_state,
 * bdmi_get_cell_indices, bdmi_get_forces, bdmi_visible_vertices (and bdmi_render_flock) - refuse it with -1 before
 * anything is launched or written; read a slab with bdmi_slab_get.  bdmi_grid_info, the timers, bdmi_sync and
 * bdmi_step work on both kinds of handle. */
bdmi_flock *bdmi_create_slab(int64_t n, const double *positions_xyz, const double *velocities_xyz, const double *colors_rgb,
                             const int32_t *global_ids, int64_t capacity, const double *params11, double x_lo, double x_hi,
                             int has_left_neighbour, int has_right_neighbour, int device);
int64_t bdmi_slab_count(bdmi_flock *f);
int bdmi_slab_export(bdmi_flock *f, void *dev_left_rows, int64_t *n_left, void *dev_right_rows, int64_t *n_right);
int bdmi_slab_import(bdmi_flock *f, const void *dev_rows, int64_t count);
int bdmi_slab_get(bdmi_flock *f, double *rows10, int64_t capacity, int64_t *count);

/* ---- render-side reduction ------------------------------------------ */
/* Flock._compute_visibility + _build_vertices on the device (flock.py:680-728): frustum test of
 * compute_visibility_numba (:311-348; z < 0.5 or z > fog_end hidden), np.where order (ascending
 * boid index), then build_vertices_numba (:351-447): 6 float32 vertices + 6 float32 colours per
 * visible boid.  cam12 = {cam_pos, cam_forward, cam_right, cam_up}; tan_h / tan_v as the caller
 * derives them from (fov, aspect, fov_margin).  *count = visible boids; at most capacity_boids of
 * them are copied out ((count*6, 3) rows each).  Only the visible part crosses PCIe. */
int bdmi_visible_vertices(bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end,
                          double cone_length, double cone_radius, float *out_vertices, float *out_colors,
                          int64_t capacity_boids, int64_t *count);

/* ---- headless flock renderer (csrc/raster.hip; boids/render.py, tools/flock_video.py) -------------------------------
 * Image semantics of a flock frame: the image fixed-function GL draws for the reference's Flock.draw (flock.py:730-782
 * under core/application.py:44-95): opaque flat-coloured GL_TRIANGLES, GL_DEPTH_TEST (GL_LESS, depth writes on), linear
 * fog towards the clear colour, gluLookAt + gluPerspective.  Where GL leaves the result to the implementation, one
 * deterministic answer is fixed here; the kernels and the tests' NumPy restatement (tests/raster_ref.py) both follow
 * this text.  Arithmetic is float64 in the order written, without FMA; the edge functions are exact integers.
 *
 * Input: vertices and colors, float32 (3T, 3); triangle t = rows 3t, 3t+1, 3t+2 (what bdmi_visible_vertices
 * returns).  The colour of triangle t is the colour row of its first vertex.
 * params (17 doubles): eye[3], target[3], up[3], fovy (degrees, in (0, 180); reference 90), near (0.1), far (1000),
 * fog_start (50), fog_end (800), bg[3] (in [0, 1]; reference (0.01, 0.01, 0.02)).  near > 0, far > near and
 * fog_end > fog_start are required (NBMI_ERR_ARG otherwise, as for any value that is not finite).
 * View constants f, s, u, cot, aspect, za, zb and, per vertex, x_e, y_e, z_e, x_c, y_c, z_c, w_c exactly as in the
 * point renderer's text (include/nbmi.h: same formulas, same association), p = the float32 vertex converted exactly.
 *
 * Per triangle:
 *   discarded whole if any coordinate of any vertex is not finite, if any vertex has w_c < near, or if any vertex has
 *     z_c > w_c.  (GL would clip at the near and far planes instead.  A boid that passes the reference's visibility
 *     test has 0.5 <= z <= far at its centre and its cone reaches 1.2 further, so this touches only cones within 1.3
 *     of the camera plane or of the far plane.)
 *   x_w = (x_c / w_c)(W / 2) + W / 2, y_w = (y_c / w_c)(H / 2) + H / 2 per vertex; discarded whole if any |x_w| or
 *     |y_w| exceeds 2^20
 *   snap to 4 sub-pixel bits: X = floor(x_w 16 + 0.5), Y = floor(y_w 16 + 0.5) as int64.  Everything on X, Y below is
 *     exact integer arithmetic (|X|, |Y| <= 2^24, so every product and every E stays below 2^52 and converts to
 *     float64 exactly)
 *   area2 = (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0).  Zero: discarded.  Negative: vertices 1 and 2 change places
 *     (no face culling: both windings are drawn), so that area2 > 0
 *   pixel (i, j), 0 <= i < W, 0 <= j < H, is sampled at its centre P = (16 i + 8, 16 j + 8).  For the edge from vertex
 *     b to vertex c opposite vertex a ((b, c) = (1, 2), (2, 0), (0, 1) for a = 0, 1, 2), dx = Xc - Xb, dy = Yc - Yb:
 *       E_a = dx (P_y - Y_b) - dy (P_x - X_b)
 *     The pixel is covered iff for every edge E_a > 0, or E_a == 0 and the edge owns its points:
 *     dy < 0 or (dy == 0 and dx > 0).  Two triangles that share an edge cover a pixel centre on it exactly once.
 *   depth: l_a = double(E_a) / double(area2), z_n = z_c / w_c per vertex, z_f = (l_0 z_n0 + l_1 z_n1) + l_2 z_n2,
 *     d = floor((z_f 0.5 + 0.5)(2^24 - 1) + 0.5).  A covered pixel with 0 <= d < 2^24 - 1 is a fragment.
 * The fragment that wins pixel (i, j) is the one with the smallest (d, t) in lexicographic order: GL_LESS against a
 * depth buffer cleared to 2^24 - 1 with the triangles drawn in row order, so among equal depths the first drawn stays.
 * Its colour: w_f = 1 / ((l_0 / w_c0 + l_1 / w_c1) + l_2 / w_c2) (the eye-space depth at the pixel),
 *   fog = clamp((fog_end - w_f) / (fog_end - fog_start), 0, 1), C = clamp(colour, 0, 1) (NaN -> 0),
 *   C' = fog C + (1 - fog) bg, channel = floor(C' 255 + 0.5).  Pixels without a fragment get floor(bg 255 + 0.5).
 * Output uint8 (H, W, 3) RGB with row 0 at the TOP: window pixel (i, j) is image row H - 1 - j, as the point renderer.
 * Only correctly rounded float64 operations and exact integers take part (there is no exp here), so the device image
 * equals the restatement byte for byte, fog included, and is the same bytes on every run.
 * Two deviations from GL: near / far clipping is replaced by the whole-triangle discard above, and depth and fog are
 * interpolated as written rather than by an implementation's fixed-point set-up.
 * Not drawn: the reference's wireframe cube (rendering/grid.py, twelve GL_LINES) and its HUD text.
 *
 * Both calls draw with an nbmi_render handle of include/nbmi.h (one per output size; its z-buffer is allocated at the
 * first triangle frame) and return when the image is in out_rgb (W*H*3 bytes).  At most 2^31 - 1 triangles; zero
 * triangles, or all discarded, give the background image.  A frame whose triangles with a box of more than 64 pixel
 * centres number 2^28 - 1 or more, or whose boxes sum to 2^36 or more chunks of 32 x 8 pixels, is refused with
 * NBMI_ERR_CAPACITY.
 * After a triangle frame nbmi_render_stats gives {triangles drawn (not discarded, area2 != 0), fragments, winning
 * fragments, pixels with a fragment} (the last two are equal here) and nbmi_render_timers gives
 * {project + rasterise, 0, resolve, copy to the host} (the resolve kernel packs the RGB8 rows itself). */
typedef struct nbmi_render nbmi_render; /* as in nbmi.h; a repeated typedef is legal C11 / C++ */
/* Host arrays (3 triangles, 3) float32 each, uploaded through pinned staging. */
int bdmi_render_triangles(nbmi_render *r, const float *vertices_xyz, const float *colors_rgb, int64_t triangles,
                          const double *params17, uint8_t *out_rgb);
/* The frame Flock.draw would put on the screen: visibility and cone building of bdmi_visible_vertices (same arguments,
 * same masks, same float32 vertices, ascending boid order) left on the device and rasterised there; only the image
 * crosses PCIe.  The image equals bdmi_render_triangles of what bdmi_visible_vertices returns for these arguments.
 * *visible_boids (may be NULL) = the visible count.  The handle and the renderer must be on the same device; slab
 * handles (bdmi_create_slab) are refused with NBMI_ERR_ARG.  The flock's state is not touched. */
int bdmi_render_flock(nbmi_render *r, bdmi_flock *f, const double *cam12, double tan_h, double tan_v, double fog_end_vis,
                      double cone_length, double cone_radius, const double *params17, uint8_t *out_rgb,
                      int64_t *visible_boids);

#ifdef __cplusplus
}
#endif
#endif /* BDMI_H */
