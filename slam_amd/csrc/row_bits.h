// The packed row word of an observation packet, as the kernels (kernels.h) and the host's row book (rows.h) both read it.
#pragma once

namespace slamgpu {

constexpr int kRowLiveBit = 1 << 30;  // packet row[k]: the landmark's live record buffer rides in bit 30 of its genealogy row
constexpr int kRowFreshBit = 1 << 29; // packet row[k]: the landmark was written by the PREVIOUS update and nothing has composed its
                                      // row since (the resample this launch applies excepted): its record sits in the source
                                      // slot itself, no genealogy lookup needed -- the usual case for a landmark in view
constexpr int kRowMask = kRowFreshBit - 1;

}  // namespace slamgpu
