/*
 * druggen_hip_text.h -- the text-producing entries of libdruggen_hip.so (gfx950 / MI355X): what the library writes for
 * people and other tools to read, next to the numeric C ABI of druggen_hip.h.  Same conventions (device pointers, the
 * caller's stream, 0 / DG_E_* / hipError_t return values, dg_last_error_string()).  A second header because the first one is
 * pinned, prototype by prototype, to DG_VERSION 232 and its ctypes table (druggen_amd/_lib.py SIGNATURES); the entries here
 * are typed from TEXT_SIGNATURES of the same file and checked the same way (tests/test_mol_smiles_host.py).
 */
#ifndef DRUGGEN_HIP_TEXT_H
#define DRUGGEN_HIP_TEXT_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- SMILES strings of decoded molecules (csrc/mol_smiles.hip) ---- */
#define DG_SMILES_FORMS 2         /* scope (after DG_CANON_WHOLE 0 / DG_CANON_LARGEST 1): every atom whose label is not 0xFF */
#define DG_SMILES_NO_GRAPH (-2)   /* length: the bond list was truncated (n_bonds > cap) or flags < 0 */
#define DG_SMILES_RINGS    (-3)   /* length: more than 99 ring closures open at once */
#define DG_SMILES_LONG     (-4)   /* length: the string is longer than str_cap */
#define DG_SMILES_MAX_LDS  49152  /* bytes of adjacency rows + label triangle + string one molecule may take */

/* dg_mol_smiles: one SMILES string per molecule of a batch, written on the device.  One wave per molecule; the graph and
 * the string live in LDS, the search is serial, the batch is parallel.  Integers only, no atomics on global memory, no host
 * synchronisation (capturable), nothing allocated.
 *
 * The graph: atoms [B,N] u8 labels, bonds [B,cap,4] u8 rows (hi, lo, label, 0) (4-byte aligned), n_bonds [B] -- as
 * dg_decode_graph or dg_mol_canon (canon_atoms, canon_bonds, n_bonds_in) wrote them.  `scope` selects the atoms:
 * DG_CANON_LARGEST those with component[b,i] == largest[b]; DG_CANON_WHOLE every atom except isolated pads (label 0 and no
 * bond row); DG_SMILES_FORMS every atom whose label is not 0xFF.  component / largest are read under DG_CANON_LARGEST only.
 * Only rows with both ends in the scope count (rows with hi == lo or an end >= N are skipped; the decode lists none, and no
 * pair twice).  flags [B] (may be NULL): a negative value means the molecule has no graph (n_splits of dg_mol_canon).
 *
 * The tables (device memory, made by the host; the kernel knows no chemistry):
 *   atom_table [n_atom_labels,4] u8: two symbol characters (the second 0 if none), a flag byte -- bit 0: written in
 *     brackets, bit 1: may be written lower-case -- and 0;
 *   bond_table [n_bond_labels,2] u8: the symbol character and an is-aromatic flag.
 * A label without a table row, or whose symbol character is 0, is written `?` (no reader accepts it).
 *
 * Traversal.  Components in ascending order of their smallest atom index, joined with `.`.  In a component a depth-first
 * search from the smallest index visiting neighbours in ascending index: the preorder, each atom's parent and its tree
 * children in discovery order.  Every other bond is a ring bond; it joins an atom to one of its ancestors.
 * Grammar.  An atom is lower-case when its table flag allows it and one of its bonds is aromatic.  Between two lower-case
 * atoms an aromatic bond is omitted and every other bond written (`-` for single); between any other pair a bond whose
 * symbol is `-` is omitted and the rest written.  At an atom: the symbol of the bond to its parent, the atom (`C`, `Cl`,
 * `c`, `[Se]`, `[se]`, `*`), its ring-bond digits, its children -- every child but the last in parentheses.  Ring-bond
 * digits in the order of the other end's preorder position (closings first); a closing writes the bond's symbol before its
 * number, an opening none; an opening takes the smallest free number from 1; a number closed at an atom is free again from
 * the next atom on; 1..9 as one digit, 10..99 as `%nn`.  No hydrogens, charges, isotopes or chirality; bracket atoms bare.
 *
 * Outputs, every element stored by every call:
 *   length [B]: >= 0 the string's length; DG_SMILES_NO_GRAPH; DG_SMILES_RINGS (it outranks DG_SMILES_LONG); DG_SMILES_LONG;
 *   n_written [B]: atoms of the scope (0 without a graph);  order [B,N] u8: the atom index of the k-th atom of the
 *   traversal, 0xFF past n_written -- reported for DG_SMILES_RINGS / _LONG too;
 *   text [B,str_cap] u8: ASCII, zeros past length, all zeros when length < 0.
 *
 * B < 0, N outside 1..256, cap < 0, str_cap < 1, n_atom_labels outside 1..255, n_bond_labels outside 1..256, or
 * 4 N ceil(N / 32) + N (N - 1) / 2 + str_cap (each rounded up to 4) above DG_SMILES_MAX_LDS: DG_E_SHAPE; a scope other than
 * 0 / 1 / 2, a null pointer (bonds may be NULL when cap == 0, component / largest unless scope == 1, flags always) or a
 * misaligned one (bonds and the int arrays: 4 bytes): DG_E_ARG.  The shape is checked first, then the scope.  B == 0
 * returns 0 without a launch. */
int dg_mol_smiles(const unsigned char* atoms, const unsigned char* bonds, const int* n_bonds, const unsigned char* component,
                  const int* largest, const int* flags, const unsigned char* atom_table, int n_atom_labels,
                  const unsigned char* bond_table, int n_bond_labels, int B, int N, int cap, int scope, int str_cap,
                  int* length, int* n_written, unsigned char* order, unsigned char* text, dg_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DRUGGEN_HIP_TEXT_H */
