// lab/small_lab.inc -- laboratory build only (-DSPANAGG_AB, libspanagg_ab.so):
// the small-table ablation instance.  Included by spanagg_kernels.hip; the
// product library never compiles it.
//
// An engine created with SA_DIAG_* flags runs the generic 1,024-thread v2
// kernel with V2Plain's switches plus DIAG (honour the ablation bits, stamp
// the step's segments); sa_create gives such an engine SmallKernel::Generic1024
// and refuses the flags on the linear-threshold kernel, which has no ablation
// instance.
struct V2Diag : V2Plain {
  static constexpr bool DIAG = true;
};

static const void *small_fn(SmallKernel k, bool diag) {
  return diag ? (const void *)&ingest_v2_kernel<0, 0, 0, false, 1024, V2Diag> : product_small_fn(k);
}
