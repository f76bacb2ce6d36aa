// TEST-ONLY: the emulator (emu.cpp, unchanged) built a second time with the lean probe body's CACHED form — the wave's LDS cache of overflow
// look-ups, its token election and its two syncs: what every list in locus order and every rest list of the locus path runs on the device —
// as the form its driver instantiates (dbtk_probe2.h: DBTK_P2_DEFAULT_CACHE).  Compiled by tests/test_probe_unsorted.py itself.
#define DBTK_P2_DEFAULT_CACHE true
#include "emu.cpp"
