/* Host lists over CSR index spaces, shared by the aggregation preconditioners (pc_amgx.c, pc_twolevel.c): members of an
 * aggregate, rows of a colour, fine nonzeros summed into a coarse nonzero -- all "items grouped by a key" -- and the
 * position of a column in a sorted row. */
#ifndef DFL_CSR_LISTS_H
#define DFL_CSR_LISTS_H
#include <stdlib.h>
#include <string.h>
#include "dedflow.h"

/* Stable bucket fill (counting sort): item[off[b] .. off[b+1]) = the i in [0, n) with key[i] == b, ascending.
 * Every key lies in [0, nbucket).  Allocates off[nbucket+1] and item[max(n, 1)]; the caller frees both. */
static void csr_bucket_fill(index_type n, const index_type* key, index_type nbucket, index_type** off_out,
                            index_type** item_out) {
    index_type* off = (index_type*)calloc((size_t)nbucket + 1, sizeof(index_type));
    index_type* item = (index_type*)malloc(sizeof(index_type) * (size_t)(n > 0 ? n : 1));
    index_type* cur = (index_type*)malloc(sizeof(index_type) * (size_t)(nbucket > 0 ? nbucket : 1));
    for (index_type i = 0; i < n; ++i) off[key[i] + 1]++;
    for (index_type b = 0; b < nbucket; ++b) off[b + 1] += off[b];
    memcpy(cur, off, sizeof(index_type) * (size_t)nbucket);
    for (index_type i = 0; i < n; ++i) item[cur[key[i]]++] = i;
    free(cur);
    *off_out = off;
    *item_out = item;
}

/* position of column j in row i (columns ascending), -1 if not stored */
static inline index_type csr_find(const index_type* rp, const index_type* ci, index_type i, index_type j) {
    index_type lo = rp[i], hi = rp[i + 1] - 1;
    while (lo <= hi) {
        const index_type mid = lo + (hi - lo) / 2;
        if (ci[mid] == j) return mid;
        if (ci[mid] < j) lo = mid + 1;
        else hi = mid - 1;
    }
    return -1;
}

#endif
