/*
 * druggen_hip_sub.h -- the substructure entry of libdruggen_hip.so (gfx950 / MI355X): a table of small pattern graphs matched
 * against every valid molecule of a batch.  Two products: per-pattern anchor counts (functional groups, alerts) and an ordered
 * first-match atom typing with additive integer values (a Wildman-Crippen style logP from a host-made table).  Same conventions
 * as druggen_hip.h (device pointers, the caller's stream, 0 / DG_E_* / hipError_t return values, dg_last_error_string()).  A
 * sixth header because the first four are pinned, prototype by prototype, to DG_VERSION 232 and the fifth to its one entry; the
 * entry here is typed from SUB_SIGNATURES of druggen_amd/_lib.py and checked the same way (tests/test_mol_sub_host.py).
 */
#ifndef DRUGGEN_HIP_SUB_H
#define DRUGGEN_HIP_SUB_H

#include "druggen_hip_desc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- substructure patterns on valid molecules (csrc/mol_sub.hip, csrc/mol_sub.h) ---- */
#define DG_SUB_MOL_FIELDS      8             /* int32 entries of a row of `mol` */
#define DG_SUB_MAX_ATOMS       16            /* atoms of a pattern */
#define DG_SUB_MAX_CLOSURES    8             /* closure bonds of a pattern */
#define DG_SUB_MAX_PATTERNS    1024          /* rows of the pattern table */
#define DG_SUB_MAX_STEPS       4096          /* the step count at which a search is given up (OVER) */
#define DG_SUB_MAX_NEIGHBOURS  8             /* neighbours kept per atom */
#define DG_SUB_PATTERN_WORDS   80            /* u32 per pattern: 8 header + 16 x 4 atom + 8 closure words */
#define DG_SUB_TYPING          1             /* flags bit 0: the pattern is a typing row */

/* dg_mol_substructure: per molecule of a batch that dg_mol_descriptors has described, how many atoms each pattern of a table
 * matches at, and the first typing pattern that matches at each atom with the sums of its values.  One workgroup per molecule,
 * the graph in LDS, the (pattern, anchor) pairs strided over the threads; integers only, no atomics on global memory, no host
 * synchronisation (capturable), nothing allocated, nothing waits on another workgroup.  This is the project's own, exactly
 * specified matcher: NOT RDKit's SMARTS engine -- no recursive environments, charges, isotopes or chirality, a bounded search,
 * and hydrogen, bond-count and ring properties as dg_mol_validity / dg_mol_descriptors define them.
 *
 * The chain is dg_decode_graph -> dg_mol_validity -> dg_mol_descriptors -> dg_mol_substructure on the SAME batch and cap.
 * Inputs: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B], as dg_decode_graph
 * wrote them; and of dg_mol_descriptors' outputs desc [B,DG_DESC_FIELDS] i32 (only the status, entry 0, is read), atom_key
 * [B,N] u32 and bond_class [B,cap] u8.  The tables (device memory, made by the host; the kernel knows no chemistry):
 *   bond_table [n_bond_labels] u32: order | aromatic << 8, the table of dg_mol_validity.
 *   atom_sets  [n_atom_labels] u32: 32 host-defined sets per atom label (typically one bit per element, then group bits).
 *   patterns   [n_patterns, DG_SUB_PATTERN_WORDS] u32, 0 <= n_patterns <= DG_SUB_MAX_PATTERNS; the record is below.
 *
 * The scope is derived, not passed.  status[b] = desc[b,0].  For a molecule of status 0:
 *   an atom a is in the scope iff atom_key[b,a] != DG_DESC_NO_KEY;
 *   a row k < min(n_bonds, cap) of the bond list is a BOND iff bond_class[b,k] & DG_DESC_BOND.
 * Per scope atom, from its key (the fields of druggen_hip_desc.h): h = key >> 8 & 15, n1 = key >> 12 & 15, n2 = key >> 16 & 7,
 * n3 = key >> 19 & 3, na = key >> 21 & 7, r3 = key >> 24 & 1; deg = n1 + n2 + n3 + na; ringed = 1 iff the atom has a BOND with
 * DG_DESC_RING_BOND; label = atoms[b,a]; sets = atom_sets[label].  Per BOND, with the bond_table word of its label:
 * kind = (aromatic ? 3 : order - 1) + 4 * (bond_class & DG_DESC_RING_BOND ? 1 : 0), so 0 single, 1 double, 2 triple, 3 aromatic
 * outside every ring, 4..7 the same in a ring.  The neighbours of an atom are the other ends of its BONDS.
 *
 * Arrays outside the definition (a record of another batch, a table of other decoders): the result then has no meaning, but the
 * kernel stays inside its arrays.  A row with an end >= N, with hi == lo, with an end outside the scope, or whose label is
 * >= n_bond_labels or has an UNKNOWN table word (order 0 or > 3, bits above 8, aromatic with order != 1) is skipped; only
 * DG_SUB_MAX_NEIGHBOURS neighbours of an atom are kept, the others are dropped (a valid molecule has at most 8: the valence
 * bound of dg_mol_validity); a label >= n_atom_labels has set word 0.
 *
 * A pattern is a connected graph of 1 <= n <= DG_SUB_MAX_ATOMS atoms in depth-first preorder: atom k > 0 has parent[k] < k and
 * a tree-bond mask of 8 bits, bit `kind` set iff a BOND of that kind is admitted; and 0 <= c <= DG_SUB_MAX_CLOSURES closure bonds
 * (k, j < k, mask) sorted by k.  Every atom predicate is a conjunction of allowed-value masks; scope atom x satisfies it iff
 *   sets[x] & sets_any != 0,            h_mask bit h[x] (bits 0..8),       deg_mask bit deg[x] (bits 0..8),
 *   n2_mask bit n2[x] (bits 0..4),      n3_mask bit n3[x] (bits 0..2),     arom_mask bit (na[x] > 0) (bits 0..1),
 *   ring_mask bit ringed[x] (bits 0..1),                                   r3_mask bit r3[x] (bits 0..1)
 * are all set.  A value past a mask's width matches nothing; mask bits past the width are ignored.
 *
 * The record of a pattern, DG_SUB_PATTERN_WORDS u32:
 *   word 0       n | c << 8 | flags << 16         (flags bit 0: DG_SUB_TYPING)
 *   words 1..4   value[0], value_h[0], value[1], value_h[1]     (int32 bit patterns)
 *   words 5..7   0
 *   words 8 + 4 k .. 11 + 4 k, for atom k = 0..15 (zeros past n):
 *       sets_any;     h_mask | deg_mask << 16;     n2_mask | n3_mask << 8 | arom_mask << 12 | ring_mask << 14 | r3_mask << 16;
 *       parent[k] | tree-bond mask << 8  (0 for atom 0)
 *   words 72..79 closure i = 0..7 (zeros past c): k | j << 8 | mask << 16
 * The kernel reads n as min(max(n, 1), 16), c as min(c, 8) and every atom index of the record modulo 16; a record that breaks
 * parent[k] < k or j < k is the host's error (druggen_amd/substructure.py builds none).
 *
 * A MATCH of pattern p anchored at scope atom a is an injective map m of the pattern's atoms to scope atoms with m(0) = a, every
 * atom predicate satisfied by its image, and for every tree bond (parent[k], k) and every closure (k, j) a BOND between the
 * images whose kind bit is set in the bond's mask.  A monomorphism, as in SMARTS: further bonds between the images do not matter.
 *
 * The search is specified, because its cost is bounded and the bound is part of the result.  Testing atom 0 against a is step 1;
 * if it fails there is no match; if n == 1 that is a match.  Then depth first: for k = 1 .. n - 1 the candidates for m(k) are the
 * neighbours of m(parent[k]) in ascending atom index.  Examining a candidate is one step: the count goes up by one, and if it is
 * then DG_SUB_MAX_STEPS the search stops and the pair (p, a) is OVER -- it counts as no match and is counted in n_over.  Else the
 * candidate is taken iff it is not the image of an atom < k, the tree-bond mask admits the kind of the BOND it was reached by,
 * predicate k holds for it, and every closure (k, j) finds a BOND between it and m(j) of an admitted kind.  A taken candidate for
 * k = n - 1 is a match; for k < n - 1 the search goes on with the first candidate of k + 1.  When the candidates of k run out
 * the search returns to k - 1 and its next candidate; when those of k = 1 run out there is no match.  A search that ends does
 * so after at most 4095 steps.  Where 4096 comes from: a 16-atom chain of wildcards whose last atom can never match (a full
 * enumeration) costs at most 443 steps from any atom of the eight drug-like molecules of tests/golden/chembl_like_smiles.csv;
 * from the centre of a square lattice of degree-4 atoms such a chain costs 4869 steps at 8 atoms and 37177 at 10.  Real
 * molecules keep a factor of nine; only lattice-like graphs run out.
 *
 * Outputs, every element stored by every call:
 *   mol [B,8] i32: status; and for status 0 -- all of them 0 otherwise --
 *       n_heavy         the atoms of the scope;
 *       n_typed         the scope atoms with a type;         n_untyped   those without;
 *       sum0, sum1      sum_c = the sum over the typed atoms a, of type t, of value[t][c] + h[a] * value_h[t][c], modulo 2^32;
 *       n_patterns_hit  the patterns with hits > 0;
 *       n_over          the pairs (p, a), a in the scope, whose search was OVER.
 *   hits [B,n_patterns] i32: the number of scope atoms a at which pattern p has a match (anchors, not matches: the count does not
 *       depend on the pattern's symmetries and needs no enumeration); 0 for any status but 0.
 *   atom_type [B,N] i32: the lowest p with DG_SUB_TYPING that has a match anchored at a; -1 if there is none, outside the scope,
 *       and everywhere for any status but 0.
 * All outputs are functions of the input alone: pinned values.
 *
 * B < 0, N outside 1..256, cap < 0, n_atom_labels outside 1..255, n_bond_labels outside 1..256 or n_patterns outside
 * 0..DG_SUB_MAX_PATTERNS: DG_E_SHAPE; a null pointer (bonds and bond_class may be NULL when cap == 0, patterns and hits when
 * n_patterns == 0) or a misaligned one (bonds, n_bonds, desc, atom_key, the three tables, mol, hits, atom_type: 4 bytes):
 * DG_E_ARG.  The shape is checked first.  B == 0 returns 0 without a launch. */
int dg_mol_substructure(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const int* desc,
                        const unsigned* atom_key, const unsigned char* bond_class, const unsigned* bond_table, int n_bond_labels,
                        const unsigned* atom_sets, int n_atom_labels, const unsigned* patterns, int n_patterns, int B, int N,
                        int cap, int* mol, int* hits, int* atom_type, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_SUB_H */
