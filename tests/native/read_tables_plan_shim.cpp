// catfish_amd/csrc/read_tables_plan.hpp (the index rules of the read-table kernels: plain C++, no device work) behind a C ABI, for
// tests/test_read_tables_plan.py:
//   g++ -std=c++17 -O1 -g -shared -fPIC ...
#include "../../catfish_amd/csrc/read_tables_plan.hpp"

extern "C" {
int shim_piece() { return RT_PIECE; }
int shim_window() { return RT_WINDOW; }
long long shim_skip() { return RT_SKIP; }
long long shim_n_pieces(long long n) { return rt_n_pieces(n); }
// out[4]: first_lo, first_hi, lab_lo, lab_hi
void shim_piece_of(long long o, long long n, long long p, long long* out) {
    const rt_piece pc = rt_piece_of(o, n, p);
    out[0] = pc.first_lo; out[1] = pc.first_hi; out[2] = pc.lab_lo; out[3] = pc.lab_hi;
}
long long shim_label_src(long long o, long long n, long long p, long long i) { return rt_label_src(rt_piece_of(o, n, p), i); }
unsigned shim_quota(int mode, long long value, unsigned m, unsigned n_pos) { return rt_quota(mode, value, m, n_pos); }
unsigned shim_read_key(unsigned seed, long long rho) { return rt_read_key(seed, rho); }
unsigned shim_perm(unsigned i, unsigned n, unsigned key) { return rt_perm(i, n, key); }
void shim_perm_many(const unsigned* i, int count, unsigned n, unsigned key, unsigned* out) {
    for (int a = 0; a < count; ++a) out[a] = rt_perm(i[a], n, key);
}
int shim_neg_selected(unsigned j, unsigned m, unsigned q, unsigned key) { return rt_neg_selected(j, m, q, key) ? 1 : 0; }
long long shim_count_slot(long long rho, long long n_reads, int which) { return rt_count_slot(rho, n_reads, which); }
long long shim_out_slot(long long lo, long long hi, unsigned k_local) { return rt_out_slot(lo, hi, k_local); }
int shim_row_ok(unsigned row, unsigned n) { return rt_row_ok(row, n) ? 1 : 0; }
long long shim_table_row(unsigned row, long long n_in_table) { return rt_table_row(row, n_in_table); }
long long shim_window_src(long long start, long long total) { return rt_window_src(start, total); }
long long shim_batch_dst(unsigned slot, unsigned size, unsigned t) { return rt_batch_dst(slot, size, t); }
}
