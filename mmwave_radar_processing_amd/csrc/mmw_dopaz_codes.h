// The two entries of mmw_doppler_azimuth_peaks's index tables that are no index: written by mmw_dopaz_peaks.h, read again by the
// RANSAC stage of mmw_dopaz_velocity.h.
#pragma once

namespace mmw {

constexpr int DZP_NONE = -1;            // the line has no (qualifying) peak
constexpr int DZP_UNDECIDED = -2;       // a comparison fell inside the band, or the frame holds a non-finite value

}  // namespace mmw
