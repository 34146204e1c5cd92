// Host build of the row-indexed training pass's restatement of po-brax_amd/csrc/pob_mlp.h (POB_MLP_HOST):
// mlp_forward_train_rows_ref and mlp_backward_rows_ref for ctypes.
#define POB_MLP_HOST
#include "pob_mlp.h"

extern "C" {
int mlp_rows_ref_forward_train(int n_layers, const int *sizes, int activation, int activate_final, long long M, const float *x,
                               const int32_t *idx, const float *table, float clip, const float *theta, float *y,
                               float *saved) {
  return mlp_forward_train_rows_ref(n_layers, sizes, activation, activate_final, M, x, idx, table, clip, theta, y, saved);
}
int mlp_rows_ref_backward(int n_layers, const int *sizes, int activation, int activate_final, long long M, const float *x,
                          const int32_t *idx, const float *table, float clip, const float *theta, const float *saved,
                          const float *dy, float *dtheta) {
  return mlp_backward_rows_ref(n_layers, sizes, activation, activate_final, M, x, idx, table, clip, theta, saved, dy, dtheta);
}
}
