/* druggen_hip_mol_features.h -- add-on to druggen_hip.h: batch assembly from a resident molecule store that carries a
 * feature plane (csrc/mol_gather.hip, druggen_amd/resident.py).  Conventions (pointers, status codes, stream)
 * as in druggen_hip.h; the ctypes table of this entry is druggen_amd/_lib.py::MOL_FEATURES_SIGNATURES.                    */
#ifndef DRUGGEN_HIP_MOL_FEATURES_H
#define DRUGGEN_HIP_MOL_FEATURES_H

#include "druggen_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dg_mol_gather for node matrices that are a one-hot atom type followed by F = M - atom_dim columns of exactly 0 or 1 (the
 * reference's --features, dataset.py:305-307).  The store of dg_mol_gather plus
 *   bits  [n, N, W]  u32  W = ceil(F / 32); feature column f of an atom position is bit f % 32 of word f / 32; the unused high
 *                         bits of the last word are zero
 * and each atoms[m, i] < atom_dim.  Outputs as dg_mol_gather, except
 *   x  [B, N, M]  f32  x[b, i, c] = [atoms[m, i] == c] for c < atom_dim, bit c - atom_dim of bits[m, i, :] for c >= atom_dim
 * with m = index[b].  EVERY element is written; `labels`, `a`, the clamping and counting of bad indices, the memset node on
 * `bad_index` and the alignment rules (molecule bases 4-byte aligned) are dg_mol_gather's, and so is the code that does them.
 * No load leaves the store's arrays.  Limits of dg_mol_gather, and 1 <= atom_dim <= M with W == ceil((M - atom_dim) / 32):
 * others DG_E_SHAPE; B == 0 returns 0 without a launch; a null pointer (`bits` may be NULL only when W == 0) or a misaligned
 * one (`bits`: 4 bytes): DG_E_ARG.                                                                                         */
int dg_mol_gather_features(const uint8_t* atoms, const int64_t* ptr, const uint32_t* entries, const uint32_t* bits, int64_t n,
                           const int64_t* index, int B, int N, int M, int E, int W, int atom_dim, float* a, int* labels,
                           float* x, int* bad_index, dg_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DRUGGEN_HIP_MOL_FEATURES_H */
