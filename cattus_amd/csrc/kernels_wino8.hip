// K1w8, the Winograd layer on eight waves of 128 accumulator registers (two per SIMD), was removed from the library: nothing
// selected it.  It computed the same bits as K1w and K1w4 and lost to K1w4 (30.5-31.5 us per layer against 28.8-29.2 at chess
// 256 -> 256, batch 256; DESIGN.md "K1w8", profiles/r05_w4_anatomy.txt); its source is in the history of this file.
// The file holds no code and is not compiled.  It remains because bench.py reads it by name for the identity of the kernel
// sources behind the committed traffic counters (kernels_sha256: comments do not count).
