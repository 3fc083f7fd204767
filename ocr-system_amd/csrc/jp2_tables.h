// JPEG 2000 tier-1 tables (ISO/IEC 15444-1 Annex C and D): the MQ coder's 47 probability states and the context numbering.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define JP2_HD __device__
#define JP2_TABLE static __device__ const
#else
#define JP2_HD
#define JP2_TABLE static const
#endif

// one state per word: Qe | NMPS << 16 | NLPS << 22 | SWITCH << 28   (Table C.2)
#define JP2_MQ(qe, nmps, nlps, sw) ((uint32_t)(qe) | (uint32_t)(nmps) << 16 | (uint32_t)(nlps) << 22 | (uint32_t)(sw) << 28)
JP2_TABLE uint32_t jp2_mq_states[47] = {
    JP2_MQ(0x5601, 1, 1, 1),    JP2_MQ(0x3401, 2, 6, 0),    JP2_MQ(0x1801, 3, 9, 0),    JP2_MQ(0x0AC1, 4, 12, 0),   JP2_MQ(0x0521, 5, 29, 0),
    JP2_MQ(0x0221, 38, 33, 0),  JP2_MQ(0x5601, 7, 6, 1),    JP2_MQ(0x5401, 8, 14, 0),   JP2_MQ(0x4801, 9, 14, 0),   JP2_MQ(0x3801, 10, 14, 0),
    JP2_MQ(0x3001, 11, 17, 0),  JP2_MQ(0x2401, 12, 18, 0),  JP2_MQ(0x1C01, 13, 20, 0),  JP2_MQ(0x1601, 29, 21, 0),  JP2_MQ(0x5601, 15, 14, 1),
    JP2_MQ(0x5401, 16, 14, 0),  JP2_MQ(0x5101, 17, 15, 0),  JP2_MQ(0x4801, 18, 16, 0),  JP2_MQ(0x3801, 19, 17, 0),  JP2_MQ(0x3401, 20, 18, 0),
    JP2_MQ(0x3001, 21, 19, 0),  JP2_MQ(0x2801, 22, 19, 0),  JP2_MQ(0x2401, 23, 20, 0),  JP2_MQ(0x2201, 24, 21, 0),  JP2_MQ(0x1C01, 25, 22, 0),
    JP2_MQ(0x1801, 26, 23, 0),  JP2_MQ(0x1601, 27, 24, 0),  JP2_MQ(0x1401, 28, 25, 0),  JP2_MQ(0x1201, 29, 26, 0),  JP2_MQ(0x1101, 30, 27, 0),
    JP2_MQ(0x0AC1, 31, 28, 0),  JP2_MQ(0x09C1, 32, 29, 0),  JP2_MQ(0x08A1, 33, 30, 0),  JP2_MQ(0x0521, 34, 31, 0),  JP2_MQ(0x0441, 35, 32, 0),
    JP2_MQ(0x02A1, 36, 33, 0),  JP2_MQ(0x0221, 37, 34, 0),  JP2_MQ(0x0141, 38, 35, 0),  JP2_MQ(0x0111, 39, 36, 0),  JP2_MQ(0x0085, 40, 37, 0),
    JP2_MQ(0x0049, 41, 38, 0),  JP2_MQ(0x0025, 42, 39, 0),  JP2_MQ(0x0015, 43, 40, 0),  JP2_MQ(0x0009, 44, 41, 0),  JP2_MQ(0x0005, 45, 42, 0),
    JP2_MQ(0x0001, 45, 43, 0),  JP2_MQ(0x5601, 46, 46, 0),
};
#undef JP2_MQ

// contexts: 0-8 zero coding, 9-13 sign, 14-16 magnitude refinement, 17 run length, 18 UNIFORM (Table D.7 gives their initial states)
constexpr int JP2_CX_SIGN = 9, JP2_CX_MAG = 14, JP2_CX_RUN = 17, JP2_CX_UNI = 18, JP2_NCX = 19;

// zero-coding context from the counts of significant horizontal (0-2), vertical (0-2) and diagonal (0-4) neighbours (Table D.1),
// four bits per entry so that a look-up is a shift of a constant, not a load.  LL / LH: one word per h, entry v * 5 + d (HL swaps h
// and v).  HH: one word, entry min(h + v, 2) * 5 + d.
constexpr uint64_t JP2_ZC_LH[3] = {0x444443333322210ull, 0x777777777766665ull, 0x888888888888888ull};
constexpr uint64_t JP2_ZC_HH = 0x887528874188630ull;
