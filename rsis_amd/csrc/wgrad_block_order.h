// Block order of the grouped fp32 weight-gradient launch (conv_wgrad_tiled.hip): hardware block index -> logical block index.
// The dispatcher deals block b of a launch to XCD b % 8 (observed, not a contract: it only matters for speed), so blocks b, b + 8, ...
// share one L2.  The map gives XCD x = b % 8 ONE contiguous range of the launch's n logical blocks, in the order it runs them:
//     q = n / 8, r = n % 8:  XCD x owns q + (x < r) blocks, starting at x * q + min(x, r);  logical = that start + b / 8
// -- a bijection on [0, n) for every n >= 1 (n < 8: the identity).  Neighbouring logical blocks of a job are neighbouring dW tiles of
// one split, which read the same x slab (or dy slab): on one XCD the second read is an L2 hit instead of a fetch over the fabric.
// Plain C++ on purpose: tests/test_wgrad_block_order.py compiles this header with the host compiler.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RSIS_ORDER_HD __host__ __device__
#else
#define RSIS_ORDER_HD
#endif

RSIS_ORDER_HD inline int rsis_xcd_logical_block(const int b, const int n) {
  const int x = b & 7, q = n >> 3, r = n & 7;
  return x * q + (x < r ? x : r) + (b >> 3);
}
