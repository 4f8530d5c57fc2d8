/* 4mc_amd/csrc/codec_level.h — the one level -> (codec, codec level) mapping of the file API, the CLI and the device image
 * encode (native/4mc.c:243-253 for .4mc, :411-419 for .4mz).  Internal to the library: not exported. */
#ifndef FOURMC_CODEC_LEVEL_H
#define FOURMC_CODEC_LEVEL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* returns the FOURMC_CODEC_* for `level` of a file with `magic`; *codec_level = the level the codec is called with */
__attribute__((visibility("hidden"))) int fourmc_level_codec(uint32_t magic, int level, int* codec_level);
#ifdef __cplusplus
}
#endif
#endif
