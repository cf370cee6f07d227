/*
 * druggen_hip_fp.h -- the fingerprint-producing entry of libdruggen_hip.so (gfx950 / MI355X): circular fingerprints of decoded
 * molecules, the input of dg_fp_tanimoto (druggen_hip.h).  Same conventions as druggen_hip.h (device pointers, the caller's
 * stream, 0 / DG_E_* / hipError_t return values, dg_last_error_string()).  A third header because the first two are pinned,
 * prototype by prototype, to DG_VERSION 232 and their ctypes tables (druggen_amd/_lib.py SIGNATURES / TEXT_SIGNATURES); the
 * entry here is typed from FP_SIGNATURES of the same file and checked the same way (tests/test_mol_fp_host.py).
 */
#ifndef DRUGGEN_HIP_FP_H
#define DRUGGEN_HIP_FP_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- circular fingerprints of decoded molecules (csrc/mol_fp.hip) ---- */
#define DG_FP_NO_GRAPH   (-2)   /* n_features: the bond list was truncated (n_bonds > cap) or flags < 0 */
#define DG_FP_MAX_RADIUS 4      /* radius is 0..4 */

/* dg_mol_fingerprint: one ECFP-style circular fingerprint (Rogers & Hahn 2010) per molecule of a batch, packed as
 * dg_fp_tanimoto reads it.  One workgroup per molecule; the graph lives in LDS, the batch is parallel.  Integers only, no
 * atomics on global memory, no host synchronisation (capturable), nothing allocated.  The bit positions are the project's
 * own (the hash is mix64 below), not RDKit's.
 *
 * The graph: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B] -- as
 * dg_decode_graph wrote them.  `scope` selects the atoms: DG_CANON_LARGEST those with component[b,i] == largest[b];
 * DG_CANON_WHOLE every atom except isolated pads (label 0 and no bond row).  component / largest are read under
 * DG_CANON_LARGEST only.  Only the first min(n_bonds, cap) rows are read, and only rows with both ends in the scope count:
 * these are the BONDS below (rows with hi == lo or an end >= N are skipped; the decode lists none, and no pair twice -- a
 * list that names a pair twice is outside this definition).  flags [B] (may be NULL): a negative value means the molecule
 * has no graph; so does n_bonds > cap.
 *
 * The tables (device memory, made by the host; the kernel knows no chemistry):
 *   atom_words [n_atom_labels] u32: one word per atom label (the host puts the atomic number there);
 *   bond_table [n_bond_labels,2] u32: (word, order2) per bond label (the host: the bond-type value 1 / 2 / 3 / 12 and twice
 *     the bond order 2 / 4 / 6 / 3).
 * A label without a table row takes word 0xFFFFFFFF and order2 0.
 *
 * Definition.  M(z) is splitmix64's finaliser on 64-bit unsigned integers: z += 0x9E3779B97F4A7C15;
 * z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; M = z ^ (z >> 31).  All sums are
 * modulo 2^64 (val2 is summed modulo 2^32 first).  "Bonds of a": the bonds with a as one end.
 *   Atom invariant: deg[a] the number of bonds of a; val2[a] the sum of their order2; ring[a] 1 if one of them lies on a
 *     cycle of the graph of the bonds (it is not a bridge), else 0.
 *   Layer 0: t = M(aw[label of a]); t = M(t + deg[a]); t = M(t + val2[a]); id_0[a] = M(t + ring[a]).
 *   Layer r = 1..radius: id_r[a] = M( M(id_(r-1)[a] + r) + sum over the bonds (a, x, l) of a of M(id_(r-1)[x] + M(bw[l])) ),
 *     for every atom of the scope in every layer (bw[l]: the word of bond label l).
 *   Environment: env_r[a] is the set of bonds with an end within distance r - 1 of a (distance: bonds on a shortest path;
 *     env_1[a] is the bonds of a); env_0 is empty.
 *   Feature set F, a set of 64-bit values: every id_0[a] of the scope; and for every non-empty bond set E, at the smallest r
 *     in 1..radius at which some atom has env_r[a] == E, the minimum of id_r[a] over the atoms with env_r[a] == E at that
 *     layer.  An environment already seen at a lower layer, for any atom, adds nothing; atoms without bonds contribute
 *     layer 0 only.  Equal values count once.
 *
 * Outputs, every element stored by every call:
 *   words [B, nbits / 32] i32: bit (id mod nbits) -- id as an unsigned 64-bit integer -- for every id in F; bit k is bit
 *     k % 32 of word k / 32 (the packing of dg_fp_pack);  counts [B] i32: the number of set bits;
 *   n_features [B] i32: the number of elements of F, before folding; DG_FP_NO_GRAPH for a molecule without a graph, whose
 *     words are all zero and whose count is 0.
 *
 * B < 0, N outside 1..256, cap < 0, radius outside 0..DG_FP_MAX_RADIUS, nbits not a multiple of 32 in 32..4096,
 * n_atom_labels outside 1..255 or n_bond_labels outside 1..256: DG_E_SHAPE; a scope other than 0 / 1, a null pointer (bonds
 * may be NULL when cap == 0, component / largest unless scope == 1, flags always) or a misaligned one (bonds, the tables
 * and the int arrays: 4 bytes): DG_E_ARG.  The shape is checked first, then the scope.  B == 0 returns 0 without a launch.
 * No bond count up to cap and no N up to 256 is refused: the bond list is read from global memory. */
int dg_mol_fingerprint(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const unsigned char* component,
                       const int* largest, const int* flags, const unsigned* atom_words, int n_atom_labels,
                       const unsigned* bond_table, int n_bond_labels, int B, int N, int cap, int scope, int radius, int nbits,
                       int* words, int* counts, int* n_features, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_FP_H */
