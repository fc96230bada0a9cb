/*
 * adsorbdiff_slabs.h - the C ABI of slab cutting (csrc/slabcut.hip, adsorbdiff_amd/slabs.py).
 * A companion of adsorbdiff_hip.h with the same conventions (status codes, device pointers, `stream` = hipStream_t);
 * adsorbdiff_amd/lib.py binds its prototypes from this text exactly as it binds the main header's.
 *
 * The reference's compute_slabs (placement/slab.py:485-552: pymatgen's SlabGenerator, StructureMatcher and
 * SpacegroupAnalyzer per Miller index) and get_symmetrically_distinct_miller_indices for a batch of bulks.  Neither
 * pymatgen nor spglib was run against it: parity with pymatgen unpinned; what follows is the contract.  The bulk's cell is
 * taken as given (no standardize_bulk).  All arithmetic is double; a bulk's results do not depend on the batch it is in,
 * and two runs give the same bits (no float atomics).
 *
 * A batch of B bulks: pos double [N,3] (Cartesian), cell double [B,9] (rows = lattice vectors, right-handed),
 * atomic_numbers int32 [N], atom_offset int32 [B+1]; periodic in all three directions.
 *
 * Per (bulk, Miller index h), h divided by its gcd:
 *  1. Oriented cell.  (u1, u2): a basis of the integer lattice {u : h.u = 0} from the extended Euclid algorithm,
 *     Lagrange-Gauss reduced in the Cartesian metric.  u1 is the shortest vector of that lattice; among vectors whose
 *     squared lengths differ by no more than 1e-9 L^2 (L: the cell's longest edge) the lexicographically greatest integer
 *     triple.  u2 is, among the vectors v that complete u1 to a basis with u1 x u2 = h (so that the Cartesian cross product
 *     points along the plane normal n, the direction of h in the reciprocal basis), the shortest one with
 *     u1.v <= 1e-9 |u1|^2.  Hence |u1| <= |u2| and u1.u2 <= 0 (within that tolerance), right-handed.  Where the two shortest
 *     vectors form an obtuse pair of the other hand, u2 is therefore not the second shortest vector but that minus u1.
 *     u3: the integer vector with h.u3 = 1 whose component in the plane is shortest; ties (1e-9 L^2 on the squared
 *     length) to the lexicographically greatest triple.  (u1, u2, u3) is unimodular; the height of the cell along n is
 *     d = d_hkl.
 *  2. Thickness.  n_slab = ceil(min_slab_size / d) oriented cells of slab, n_vac = ceil(min_vacuum_size / d) of vacuum.
 *     Output frame: cell[0] along +x, cell[1] in the xy plane, cell[2] = (0, 0, (n_slab + n_vac) d) - perpendicular, where
 *     pymatgen keeps the oblique u3: a stated deviation, equivalent for every consumer behind the vacuum.  The slab is
 *     centred at half that height: (lowest atom + highest atom) / 2 lies there.
 *  3. Terminations.  The heights of the oriented cell's atoms modulo d, sorted; every periodic gap above `tol` gives a cut
 *     plane at its midpoint, `shift` = that height in [0, d); a plane within 1e-9 A of d is the plane at 0.  No gap above tol: one cut, in the largest gap (ties within
 *     1e-9 A to the lowest height).  A cut's slab holds the n_slab oriented cells above the plane.
 *  4. Primitive in-plane cell.  The in-plane translations that map the oriented cell's atoms onto themselves (species equal,
 *     positions within symprec, modulo (u1, u2, u3) - for a slab of whole oriented cells these are the translations that map
 *     the slab onto itself) generate with u1, u2 a finer lattice.  Its basis (p1, p2): p1 the shortest vector, ties
 *     (1e-9 L^2) to the greatest component along u1, then the greatest across it; p2 by the rule of u2.  One atom per
 *     translation class is kept, the one of the lowest index in the bulk.  Without such translations (p1, p2) = (u1, u2).
 *     Translations that do not close to a group at this symprec refuse the bulk.
 *  5. Duplicate terminations.  Two cuts are the same slab when some (x, y) -> R (x, y) + tau, z kept relative to the slabs'
 *     mid-planes, takes every atom of one onto an atom of its species of the other within symprec, modulo (p1, p2).  R: the
 *     point operations of the lattice (p1, p2) - integer 2 x 2 matrices W (entries -2 .. 2, determinant +-1) in that basis
 *     under which |p1|, |p2| and |p1 + p2| keep their lengths within symprec, as adf_slab_symmetry_search finds them.  tau:
 *     whatever takes the first atom of the rarest species onto an atom of its species at its height.  Atoms closer than
 *     2 symprec to each other are not told apart.  The cut with the smaller shift is kept.
 *  6. Top and bottom.  A kept slab is invertible when the test of 5 maps it onto itself after z -> -z about its mid-plane
 *     (any operation with R_zz = -1).  Every kept slab is emitted with top = 1; a non-invertible one again with top = 0:
 *     turned by 180 degrees about x through its centre, cell[2] restored to +z, cell[1] negated and, where that leaves
 *     cell[0].cell[1] > 0, lowered by cell[0] (the rule of u2 once more: the cell stays right-handed and obtuse), centred and
 *     wrapped.  Flipped slabs are not compared with other terminations.
 *  7. Order.  Pairs in the caller's order.  Within a pair the top = 1 slabs by ascending shift, then the top = 0 slabs in the
 *     same order.  Atoms: wrapped to fractional in-plane coordinates in [-1e-6, 1 - 1e-6); atom a precedes atom b when it is
 *     lower by more than symprec; else (same layer) when its first fractional coordinate is smaller by more than 1e-6; else
 *     when its second is; the position of an atom is the number of atoms that precede it.
 */
#ifndef ADSORBDIFF_SLABS_H
#define ADSORBDIFF_SLABS_H

#include "adsorbdiff_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Distinct Miller indices.  The point group of each bulk: the integer matrices W with entries in {-1, 0, 1} whose rows
 * a'_i = sum_j W_ij a_j keep the lengths of the three edges and the three face diagonals within symprec, and under which
 * f -> f W + t maps the atoms onto themselves (species equal, within symprec) for some t.  The search is complete for
 * conventional and reduced cells; for other cells it can only miss operations, which splits classes: duplicate slabs later,
 * never a wrong one.  The classes: gcd-reduced h with |h|, |k|, |l| <= max_miller under h -> W h and h -> -h; the
 * representative is the lexicographically greatest member inside the box; representatives come in descending order.
 *
 * adf_distinct_millers_count: found (device) and found_host (host) int32 [3 B]: per bulk the number of indices, the order
 * of the group, error bits.  One launch, one read-back.  max_miller outside 1 .. 4, symprec not finite and positive:
 * ADF_EINVAL; a bulk with a singular, left-handed or non-finite cell: ADF_EINVAL, the message names the bulk, its atoms are
 * not read.  scratch: adf_distinct_millers_scratch(N, B) bytes, 256-byte aligned, kept for the fill.
 * adf_distinct_millers_fill: millers int32 [capacity, 3]; bulk b's indices from miller_offset[b] (int32 [B+1], the
 * exclusive scan of the counts).  capacity below the total: ADF_EOVERFLOW, nothing written. */
int64_t adf_distinct_millers_scratch(int32_t num_atoms, int32_t num_bulks);
int32_t adf_distinct_millers_count(const double* pos, const double* cell, const int32_t* atomic_numbers,
                                   const int32_t* atom_offset, int32_t num_atoms, int32_t num_bulks, int32_t max_miller,
                                   double symprec, void* scratch, int32_t* found, int32_t* found_host, void* stream);
int32_t adf_distinct_millers_fill(const void* scratch, const int32_t* found, const int32_t* found_host,
                                  const int32_t* miller_offset, int32_t num_atoms, int32_t num_bulks, int32_t max_miller,
                                  int32_t capacity, int32_t* millers, void* stream);

/* Slabs: count, then fill.  P pairs: pair_bulk int32 [P], pair_miller int32 [P,3]; pair p works in the scratch segment
 * pair_atom_offset[p] .. pair_atom_offset[p+1] (int64 [P+1]), at least its bulk's atoms long; segment_atoms: the last
 * offset.  scratch: adf_slab_cut_scratch(segment_atoms, P) bytes, 256-byte aligned, kept for the fill.
 *
 * adf_slab_cut_count: counts (device) and counts_host (host) int32 [3 P]: slabs of the pair, atoms of each of them, error
 * bits.  One launch, one read-back.  A size or tolerance that is not finite and positive: ADF_EINVAL.  h = (0,0,0), a
 * singular, left-handed or non-finite cell, a bulk without atoms, a slab beyond 2^20 atoms, translations that do not close:
 * ADF_EINVAL, the message names the bulk; the bulk's atoms are not read and its segment is not written.
 *
 * adf_slab_cut_fill: pair p's slabs are rows pair_slab_offset[p] .. of the per-slab outputs, its atoms rows
 * pair_out_offset[p] .. (int32 [P+1], int64 [P+1]: the exclusive scans of the counts and of slabs x atoms).  pos64 double
 * [atom_capacity, 3], pos32 float [atom_capacity, 3] (pos64 rounded once), atomic_numbers int32 [atom_capacity]; cell double
 * [slab_capacity, 9], millers int32 [slab_capacity, 3] (gcd-reduced), shift double, top / bulk_index / natoms int32
 * [slab_capacity].  Offsets that are not the count pass's, or that pass a capacity: ADF_EOVERFLOW, the message names the
 * bulk, nothing is written.  Two launches (the check, the fill) and one read-back. */
int64_t adf_slab_cut_scratch(int64_t segment_atoms, int32_t num_pairs);
int32_t adf_slab_cut_count(const double* pos, const double* cell, const int32_t* atomic_numbers, const int32_t* atom_offset,
                           int32_t num_atoms, int32_t num_bulks, const int32_t* pair_bulk, const int32_t* pair_miller,
                           const int64_t* pair_atom_offset, int32_t num_pairs, int64_t segment_atoms, double min_slab_size,
                           double min_vacuum_size, double tol, double symprec, void* scratch, int32_t* counts,
                           int32_t* counts_host, void* stream);
int32_t adf_slab_cut_fill(const void* scratch, const int32_t* pair_bulk, const int64_t* pair_atom_offset,
                          const int32_t* pair_slab_offset, const int64_t* pair_out_offset, int32_t num_pairs,
                          int64_t segment_atoms, double symprec, int32_t slab_capacity, int64_t atom_capacity, double* pos64,
                          float* pos32, int32_t* atomic_numbers, double* cell, int32_t* millers, double* shift, int32_t* top,
                          int32_t* bulk_index, int32_t* natoms, void* stream);

#ifdef __cplusplus
}
#endif
#endif
