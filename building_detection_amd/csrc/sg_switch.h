// The library's experiment switches: ONE table, one parse rule per kind, one read per process.
//
// Every SG_* environment variable the native code looks at has a row here and is read nowhere else (tests/test_switches_cpu.py).
// A plan and the launcher behind it ask the same accessor, so they cannot see different values; masks and clamps belong to the
// place that uses a value, never to the read.  DESIGN.md's appendix is this table (and building_detection_amd/switches.py) in prose.
//
//   sg_switch<SW_NAME>()      the value as an integer (FLAG: 1 when the variable exists; OFF0: 0 only when it is set to 0)
//   sg_switch_set<SW_NAME>()  whether the variable exists at all (switches whose default depends on the caller)
//   sg_switch_f<SW_NAME>()    the value of a DBL switch
//
// The table is immutable once read, so it does not matter that every translation unit could hold its own copy.  State that can be
// SET at run time (x6_mode() / sg_set_conv_x6()) is not kept here: it is a file-local variable of ONE translation unit, conv_igemm.hip
// (g_x6_mode, behind x6_mode()) - not a variable in a header.
#pragma once
#include <stdlib.h>

// kinds: FLAG = on when the variable exists, whatever its value; INT = atoll of the value; OFF0 = on unless set to 0;
//        DBL = atof of the value.            X(name without SG_, kind, default, effect)
#define SG_SWITCH_TABLE(X)                                                                                                          \
  X(CONV_X6, INT, 1, "arithmetic of fp32 convolutions: 0 native fp32 MFMA, 1 exact bf16x6 emulation, 2 bf16 products")              \
  X(X6_VARIANT, INT, -1, "x6 structure: 0 two workgroups per CU, 1 one double-buffered workgroup per CU; unset: by tile count")     \
  X(X6_INTERLEAVE, INT, 1, "0: staggered wave halves instead of the hand-interleaved x6 step")                                      \
  X(X6_MF16, OFF0, 1, "0: multi-tap x6 convolutions on the 32x32x16 MFMA instead of 16x16x32")                                      \
  X(X6_VPAD, INT, 1, "0: no virtual channel padding (Cin % 32 != 0 goes to the fp32-MFMA kernels)")                                 \
  X(X6_NOPATCH, FLAG, 0, "patch form of the 3x3 x6 convolution off (im2col x6 kernel instead)")                                     \
  X(X6_NOWPATCH, FLAG, 0, "patch form of the low-channel 3x3 filter gradient off (slab kernel instead)")                            \
  X(X6P_CHUNKS, INT, 1, "0: 3x3 layers of 128 ... 512 channels leave the patch kernel's 64-channel chunks for the im2col kernel")   \
  X(X6P_DELAY, INT, 0, "start offset of a CU's 2nd / 3rd patch workgroup in 10 ns ticks (-1: one K loop)")                          \
  X(X6_WIDE, INT, 2, "planes-in x6 kernel: 2 every long-K multi-tap convolution, 1 the dilated ones only, 0 none")                  \
  X(X6W_VAR, INT, 1, "planes-in x6 kernel: 1 barrier in the middle of a stage, 0 wait + barrier at its end")                        \
  X(CONV_L2, INT, 7, "bit 0 grouped tile order, bit 1 channel-block K order, bit 2 tap-inner wgrad order; unset: 7 on x6, 2 on fp32 kernels") \
  X(CONV_CB, INT, 4, "slabs per channel block of the channel-block K order")                                                        \
  X(CONV_GM, INT, 0, "> 0: row tiles per group of the grouped tile order, for every launch with two or more column tiles")          \
  X(CONV_NOSKIP, FLAG, 0, "padding-tap elimination off")                                                                            \
  X(CONV_NOTHIN, FLAG, 0, "thin 1x1 streaming kernels off")                                                                         \
  X(CONV_MAX_BYTES, INT, 0, "test hook: byte limit above which a convolution call is cut into image sub-batches (<= 0: 2 GiB)")     \
  X(WGRAD_FAST1, FLAG, 0, "aligned-slab form of the fp32 filter gradient off")                                                      \
  X(WGRAD_PLAN_RATE, DBL, 110, "planner's assumed MFMA rate (TFLOP/s) for the x6 filter gradient's split count")                    \
  X(WGRAD_PLAN_RATE_B16, DBL, 110, "planner's assumed MFMA rate (TFLOP/s) for the bf16 filter gradient's split count")              \
  X(WGRAD_PIN_SMUL, INT, 1, "planes-in filter gradient: pixel shares x n")                                                          \
  X(DGRAD_PERM2, INT, 1, "0: stride-2 dgrad rows in raster order instead of parity-class order")                                    \
  X(PW_WIDE, INT, 1, "wide pointwise kernels: 0 off, 2 every aligned 1x1 stride-1 launch (tests), 3 384-wide tiles only")           \
  X(PW_VAR, INT, 1, "pw_wide_kernel<3,float>: 1 barrier in the middle of the k-step, 0 at its end")                                 \
  X(WPW_VAR, INT, 1, "wgrad_pw_wide_kernel: 1 barrier in the middle of the k-step, 0 at its end")                                   \
  X(B16_DEEP, OFF0, 1, "0: bf16 storage on the one-plane x6 kernel instead of conv_b16_kernel")                                     \
  X(B16_KS, INT, 0, "bf16 storage: upper limit of the slab depth in 16-channel units (0: by Cin)")                                  \
  X(B16_PD, INT, 0, "conv_b16_kernel: 1 / 2 register sets of prefetched slabs for every launch (0: by shape)")                      \
  X(B16_WIDE, INT, 1, "0: bf16 storage without the 256-wide LDS-DMA kernel")                                                        \
  X(SEG_FUSED, INT, 1, "segment reductions: 0 separate finalize launch, 1 fused when one workgroup covers a column block, 2 / 3 fused for every split") \
  X(FINALIZE_LANES, INT, 16, "4: four lanes per channel in seg_finalize_kernel whatever the number of partial rows")                \
  X(BN_COLS, INT, 1, "0: flat BatchNormalization apply kernels instead of the column forms")                                        \
  X(DW_STRIP, INT, 1, "0: depthwise filter gradient on the run reducer")                                                            \
  X(DW_RR, INT, 0, "rows per run of the depthwise kernels (1, 2; 0: by shape)")                                                     \
  X(DW_FSTRIP, INT, 1, "depthwise 3x3 stride-1 stencil as column strips: 1 maps of 64 rows and more, 2 every map, 0 never")         \
  X(DW_FSTRIP_HS, INT, 0, "> 0: strip height of dw_strip_kernel (0: by map height)")                                                \
  X(X6_ABLATE, INT, 0, "timing only, results wrong: x6 kernels, 1 no global loads, 2 no split / LDS store, 4 no MFMAs, 8 no stagger / no fragment reads") \
  X(X6P_ABLATE, INT, 0, "timing only, results wrong: patch kernel, 1 no K loop, 2 no patch loads, 4 phase clocks into y, 8 no y stores") \
  X(X6W_ABLATE, INT, 0, "timing only, results wrong: planes-in x6 kernel")                                                          \
  X(CONV_ABLATE, INT, 0, "timing only, results wrong: fp32-MFMA kernels")                                                           \
  X(PW_ABLATE, INT, 0, "timing only, results wrong: pw_wide_kernel<3>, 1 no A path, 2 no B DMA, 4 no MFMAs, 8 no fragment reads, 16 no barrier") \
  X(BNB_ABLATE, INT, 0, "timing only, results wrong: BatchNormalization-backward pointwise dgrad, 2 no dz store, 4 no x load")      \
  X(B16_ABLATE, INT, 0, "timing only, results wrong: conv_b16_kernel, in a -DSG_B16_ABL build of the library only")

enum SgSwitch {
#define SG_SWITCH_ENUM(name, kind, def, effect) SW_##name,
  SG_SWITCH_TABLE(SG_SWITCH_ENUM)
#undef SG_SWITCH_ENUM
  SW_COUNT
};

enum SgSwitchKind { SG_SW_FLAG, SG_SW_INT, SG_SW_OFF0, SG_SW_DBL };

struct SgSwitchRow {
  const char* name;
  SgSwitchKind kind;
  double def;
  const char* effect;
};

struct SgSwitchValue {
  bool set;
  long long i;
  double d;
};

inline const SgSwitchRow& sg_switch_row(SgSwitch s) {
  static const SgSwitchRow rows[SW_COUNT] = {
#define SG_SWITCH_ROW(name, kind, def, effect) {"SG_" #name, SG_SW_##kind, (double)(def), effect},
      SG_SWITCH_TABLE(SG_SWITCH_ROW)
#undef SG_SWITCH_ROW
  };
  return rows[s];
}

inline SgSwitchValue sg_switch_parse(SgSwitch s) {
  const SgSwitchRow& r = sg_switch_row(s);
  const char* e = getenv(r.name);
  SgSwitchValue v = {e != nullptr, (long long)r.def, r.def};
  switch (r.kind) {
    case SG_SW_FLAG: v.i = e ? 1 : 0; break;
    case SG_SW_INT: if (e) v.i = atoll(e); break;
    case SG_SW_OFF0: v.i = (e && atoi(e) == 0) ? 0 : 1; break;
    case SG_SW_DBL: if (e) v.d = atof(e); break;
  }
  return v;
}

// read at the first use of the switch, then fixed for the life of the process
template <SgSwitch S>
inline const SgSwitchValue& sg_switch_value() {
  static const SgSwitchValue v = sg_switch_parse(S);
  return v;
}
template <SgSwitch S>
inline int sg_switch() { return (int)sg_switch_value<S>().i; }
template <SgSwitch S>
inline long long sg_switch_ll() { return sg_switch_value<S>().i; }
template <SgSwitch S>
inline bool sg_switch_set() { return sg_switch_value<S>().set; }
template <SgSwitch S>
inline double sg_switch_f() { return sg_switch_value<S>().d; }
