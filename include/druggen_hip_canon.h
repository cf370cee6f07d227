/* druggen_hip_canon.h -- add-on to druggen_hip.h: canonical forms of decoded molecules (csrc/mol_canon.hip).
 *
 * An add-on header because the table test of druggen_hip.h pins that header's prototype count; these two entries are to be
 * FOLDED INTO druggen_hip.h (and their ctypes rows into _lib.SIGNATURES) when that test is next revised.  No version bump:
 * ask the library for the symbol.  Conventions (status codes, the error string, dg_stream_t) are those of druggen_hip.h.
 */
#ifndef DRUGGEN_HIP_CANON_H
#define DRUGGEN_HIP_CANON_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DG_CANON_WHOLE   0        /* scope: every atom except isolated pads (label 0 and no bond) */
#define DG_CANON_LARGEST 1        /* scope: the atoms with component == largest */

/* dg_mol_canon: a canonical form of every molecule of the batch dg_decode_graph wrote.  One workgroup of 256 lanes per
 * molecule, integers only, no host synchronisation (capturable).  Inputs: atoms [B,N] u8, bonds [B,cap,4] u8 (4-byte
 * aligned), n_bonds [B], component [B,N] u8, largest [B] -- the fields of the decode.  `scope` selects the atom set S; only
 * bonds with both ends in S count; n = |S|.
 *
 * Refinement.  c[i] = number of atoms of S with a strictly smaller key; the start key is the atom label.  A round computes
 *   sig[i] = sum over the bonds (j, l) of i of mix64((l << 16) | c[j])  mod 2^64      (mix64: splitmix64's finaliser)
 * its key is the pair (c[i], sig[i]) in lexicographic order and the new c is again the count of strictly smaller keys.  Rounds
 * repeat until c does not change (at most n per pass).  Individualisation: while some value of c is shared, take the smallest
 * shared value, keep the atom of that cell with the smallest original index, add 1 to c of the cell's other atoms, count one
 * split and refine again (at most n - 1 splits).  c ends as a bijection S -> 0..n-1: the rank.
 *
 * Outputs, every element stored by every call:
 *   n_atoms [B] = n;  n_bonds_in [B] = bonds inside S;  n_splits [B] (0: refinement alone made the partition discrete);
 *   n_rounds [B] = refinement rounds taken, the last unchanged one of every pass included;
 *   order [B,N] u8: order[r] = original position of the atom of rank r, 0xFF past n;  canon_atoms [B,N] u8: its label, 0xFF
 *   past n;  canon_bonds [B,cap,4] u8: (hi rank, lo rank, label, 0) ascending in (hi, lo), zeros past the count;
 *   key [B] i64 = sum mod 2^64 of mix64(((pos + 1) << 32) | value) over: rank r -> (r, canon_atoms[r]), (256, n_atoms),
 *   (257, n_bonds_in), bond row k -> (258 + k, the row as a little-endian u32).
 * A truncated molecule (n_bonds > cap): n_splits = -2, n_atoms = n_bonds_in = n_rounds = 0, key = 0, filler rows.
 *
 * Equal forms (n_atoms, n_bonds_in, canon_atoms[:n], the bond rows) ARE isomorphic labelled graphs: the form is a complete
 * relabelled graph.  Isomorphic graphs get equal forms whenever the cells split above are orbits.
 *
 * B < 0, N outside 1..256, cap < 0: DG_E_SHAPE; scope not 0 / 1, a null pointer (bonds / canon_bonds may be NULL when cap == 0)
 * or a misaligned one (bonds, canon_bonds: 4 bytes; the int outputs: 4; key: 8): DG_E_ARG.  B == 0 returns 0 without a launch. */
int dg_mol_canon(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const unsigned char* component,
                 const int* largest, int B, int N, int cap, int scope, int* n_atoms, int* n_bonds_in, int* n_splits,
                 int* n_rounds, unsigned char* order, unsigned char* canon_atoms, unsigned char* canon_bonds, int64_t* key,
                 dg_stream_t stream);

/* dg_mol_canon_match: within-batch uniqueness of B forms and their membership in a stock of S forms.
 * The batch: the outputs of dg_mol_canon (key, n_atoms, n_bonds_in, n_splits, canon_atoms [B,N], canon_bonds [B,cap,4]).
 * The stock (S == 0: none, its pointers are not read): stock_keys [S] i64 = key & mask(key_bits), sorted ascending as signed
 * 64-bit integers; stock_index [S] i32: sorted position -> original index, ascending inside a run of equal keys; and the
 * stock's n_atoms, n_bonds_in, n_splits [S], canon_atoms [S,N], canon_bonds [S,stock_cap,4] in ORIGINAL order.
 *   match [B,2] i32: [b,0] duplicate_of = smallest j < b with an equal form, -1 none, -2 truncated;
 *                    [b,1] stock_hit = smallest original stock index with an equal form, -1 none, -2 truncated, -3 no stock
 *   tot [8] i64: B, n_distinct (duplicate_of == -1), n_in_stock (stock_hit >= 0), n_novel (stock_hit == -1), n_truncated,
 *                n_unsplit (n_splits == 0), 0, 0
 * A key -- masked to its low key_bits bits on both sides -- only selects candidates; the answer is the byte comparison of
 * n_atoms, n_bonds_in, canon_atoms[:n] and the bond rows, so it does not depend on key_bits.  Truncated forms of either side
 * match nothing.  Every element of match and tot is stored by every call (B == 0 writes tot); no host synchronisation.
 * B < 0, S < 0, N outside 1..256, cap < 0, stock_cap < 0: DG_E_SHAPE; key_bits outside 1..64, a null or misaligned pointer
 * (bond rows: 4 bytes; int arrays: 4; keys and tot: 8): DG_E_ARG.  The shape is checked first, then key_bits. */
int dg_mol_canon_match(const int64_t* key, const int* n_atoms, const int* n_bonds_in, const int* n_splits,
                       const unsigned char* canon_atoms, const unsigned char* canon_bonds, int B, int N, int cap,
                       const int64_t* stock_keys, const int* stock_index, const int* stock_n_atoms,
                       const int* stock_n_bonds_in, const int* stock_n_splits, const unsigned char* stock_atoms,
                       const unsigned char* stock_bonds, int S, int stock_cap, int key_bits, int* match, int64_t* tot,
                       dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_CANON_H */
