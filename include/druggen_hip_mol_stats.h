/* druggen_hip_mol_stats.h -- add-on to druggen_hip.h: per-molecule statistics of a decoded batch (csrc/mol_stats.hip,
 * DESIGN 3.24).  Conventions (pointers, status codes, stream) as in druggen_hip.h; the ctypes table of these entries is
 * druggen_amd/_lib.py::MOL_STATS_SIGNATURES.  Integer arithmetic only: every output is exact and the same from run to run. */
#ifndef DRUGGEN_HIP_MOL_STATS_H
#define DRUGGEN_HIP_MOL_STATS_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of dg_mol_stats' workspace for B molecules (their 64-bit keys); 0 for B <= 0.                                        */
size_t dg_mol_stats_workspace_bytes(int B);

/* Statistics of the B molecules dg_decode_graph wrote: atoms [B,N] u8, bonds [B,cap,4] u8, n_bonds / n_components /
 * largest_size [B] i32, valence2 [B,N] u16 (may be NULL).  Optional: the graph the batch was generated from, in_atoms [B,N] u8
 * and in_labels [B,N,N] i32 (only i > j is read), and max_valence2 [M] u16, twice the largest allowed valence per atom label
 * (0xFFFF: no limit; a label >= M has none).
 *
 * mol [B,8] i32, one row per molecule; a column is -1 where an input it needs is NULL:
 *   0 atom_types     distinct values in atoms[b, :]
 *   1 largest_size, 2 n_components, 3 n_bonds   copied
 *   4 over_valent    positions with valence2[b,i] > max_valence2[atoms[b,i]]         (needs valence2 and max_valence2)
 *   5 changed_atoms  positions with atoms[b,i] != in_atoms[b,i]                      (needs in_atoms)
 *   6 changed_bonds  pairs i > j whose listed bond label (0 when absent from the list) != in_labels[b,i,j]  (needs in_labels)
 *   7 duplicate_of   smallest j < b with the same atoms row, n_bonds and bond-list dwords; -1: none
 * A truncated molecule (n_bonds > cap) has changed_bonds = -1 and duplicate_of = -2 and is nobody's duplicate.
 * tot [16] i64: B; the sums of columns 0..6 over their entries >= 0; molecules with over_valent > 0; with changed_atoms ==
 * changed_bonds == 0; with duplicate_of == -1; truncated ones; those with n_components == 1; three zeros.
 *
 * key_bits in 1..64: a molecule's 64-bit key (an order-free sum of position-dependent mixes of its atoms, n_bonds and bond
 * rows) is masked to its low key_bits bits; keys only select the pairs that are compared byte by byte, so the result does not
 * depend on key_bits.  Every element of mol and tot is written by every call; no allocation, no synchronisation.
 * Null required pointers, bonds == NULL with cap > 0, misaligned bonds (4) / mol (16) / tot, workspace (8), key_bits outside
 * 1..64: DG_E_ARG; B < 0, N outside 1..256, cap < 0, M outside 1..256 with max_valence2: DG_E_SHAPE; workspace_bytes below
 * dg_mol_stats_workspace_bytes(B): DG_E_WORKSPACE.  The shape and key_bits are checked first.  B == 0 writes tot (all zeros)
 * and needs no other pointer.                                                                                               */
int dg_mol_stats(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* n_components,
                 const int* largest_size, const unsigned short* valence2, const unsigned char* in_atoms, const int* in_labels,
                 const unsigned short* max_valence2, int B, int N, int cap, int M, int key_bits, int* mol, int64_t* tot,
                 void* workspace, size_t workspace_bytes, dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_MOL_STATS_H */
