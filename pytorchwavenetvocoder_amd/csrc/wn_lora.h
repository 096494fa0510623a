// wn_lora.h -- low-rank adapters over the flat buffers (include/wavenet_hip.h, ABI v22): the host table and the
// launchers of wn_lora.hip.  They know nothing of the network: a table entry names a row-major [rows, cols] matrix of the model's
// flat buffers and its two factors A [rank, cols], B [rows, rank] in the adapter's flat buffer.
//
// The table (int64 words, host; the kernels read a device copy of the same words):
//   [0] WN_LORA_MAGIC  [1] entries  [2] tiles  [3] reduce blocks  [4] scratch floats  [5] model elements needed
//   [6] adapter elements needed  [7] words in all
//   8 words per entry:  w_off, rows, cols, rank, a_off, b_off, the bits of (float)scale, the entry's offset into the scratch
//   one word per tile:  entry << 32 | tile of the entry (row-major over WN_LORA_TILE x WN_LORA_TILE tiles of the matrix)
//   one word per reduce block: entry << 32 | chunk of WN_LORA_TPB adapter-gradient elements of the entry (dA first, then dB)
// Grids and every summation order follow from these words alone.
#pragma once
#include "wn_device.h"

#include "../../include/wavenet_hip.h"   // struct WnLoraEntry, WN_LORA_MAX_RANK

#define WN_LORA_MAGIC 0x41524f4c4e57L   // "WNLORA"
#define WN_LORA_HEADER 8
#define WN_LORA_ENTRY_WORDS 8
#define WN_LORA_TILE 64
#define WN_LORA_TPB 256

// Validates the entries against buffers of n_model / n_adapter elements and writes the table when `table` is not NULL and holds
// `table_words` >= the words needed.  Returns the words needed, -1 on an error with its text in err[0 .. err_len).
int64_t wn_lora_build_table(const struct WnLoraEntry* entries, int n_entries, int64_t n_model, int64_t n_adapter, int64_t* table,
                            int64_t table_words, char* err, size_t err_len);
// NULL when `table` (host) is a table of wn_lora_build_table that fits buffers of these lengths, otherwise what is wrong
const char* wn_lora_table_error(const int64_t* table, int64_t n_model, int64_t n_adapter);
// params = fmaf(scale, sum_k B[o,k] A[k,c], base) on every element of every entry: one launch over the tiles
int wn_lora_merge_launch(const float* base, float* params, const float* adapter, const int64_t* table, const long* dev_table,
                         wn_stream_t st);
// dA = scale B^T g, dB = scale g A^T: one launch over the tiles of g (partials into scratch), one that sums them in tile order
int wn_lora_project_launch(const float* grads, const float* adapter, float* adapter_grads, const int64_t* table,
                           const long* dev_table, float* scratch, wn_stream_t st);
