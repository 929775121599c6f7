// ab_kernels.hip -- the split-kernel shapes of the studies (rounds 1-6) that
// the product library does not dispatch, built only into the A/B library
// (`make -C congestion-control-with-bittorren_amd ab` ->
// build-ab/libsha1chunk.so + libsha1chunk_hip.so, selected with
// SHA1CHUNK_LIB; forced with SHA1CHUNK_SPLIT_UNIT).  Not part of the product:
// these strong definitions replace the product's weak launch_split_study /
// split_unit_study_built (csrc/sha1_kernels.hip), and the shapes come from
// the same templates as the product's (csrc/sha1_split.hpp).  Results:
// profiles/sweep_r01.json, split_variants_r01.json, split_2prod_sweep_r01.json,
// split_unit_ab_r03.json.  Variants that needed code paths of their own and
// lost left the source (see the comment at the shape flags).  Every shape is
// launched through launch_shape, with the block size it was compiled for.
#include "../congestion-control-with-bittorren_amd/csrc/sha1_split.hpp"

namespace {
constexpr int kStudyUnits[] = {2, 3, 20, 21, 24, 30, 31, 34, 44, 45, 504, 505, 569, 577, 585,
                               8, 9, 10, 12, 13, 16, 17, 86, 87, 92, 97, 99, 417, 816, 817};
}

bool split_unit_study_built(int u) {
    for (int b : kStudyUnits)
        if (u == b) return true;
    return false;
}

hipError_t launch_split_study(const BatchArgs& A, int unit, hipStream_t st) {
    if (A.n == 0) return hipSuccess;
    const uint32_t groups = (A.n + 63u) / 64u;
    if (split_unit_study_built(unit)) count_launch(kLaunchStudy);
    switch (unit) {
    case 2: launch_shape<2, 1>(A, groups, st); break;
    case 3: launch_shape<3, 1>(A, groups, st); break;
#define SPLIT_V(U, V) \
    case 10 * U + V: launch_shape<U, 1, V>(A, groups, st); break;
    // unit 10*U + V, V = kVWK | kVUnmask bits, one producer
    SPLIT_V(2, 0) SPLIT_V(2, 1) SPLIT_V(2, 4) SPLIT_V(3, 0) SPLIT_V(3, 1) SPLIT_V(3, 4)
    SPLIT_V(4, 4) SPLIT_V(4, 5)
#undef SPLIT_V
    // two producer waves per consumer, 4-block units: unit 500 + V
    case 504: launch_shape<4, 1, 4, 2>(A, groups, st); break;
    case 505: launch_shape<4, 1, 5, 2>(A, groups, st); break;
    case 569:  // 500 + (kVWK | kVUnmask | kVSkipWave2): producers on waves 1 and 3
        launch_shape<4, 1, 69, 2>(A, groups, st);
        break;
    case 577:  // 569 + kVRead10 (the product's case 4 without shared loads)
        launch_shape<4, 1, 77, 2>(A, groups, st);
        break;
    case 585:  // the product's case 4 with schedule reads in four bursts of 5
        launch_shape<4, 1, (77 & ~kVRead10) | kVCoop, 2>(A, groups, st);
        break;
    case 92:  // round 5: the product's uniform case 11 with two read bursts of 10
        launch_shape<2, 2, (kSplit8V & ~kVCoop) | kVRead10, 2>(A, (groups + 1) / 2, st);
        break;
    // probes (barrier-wait and loop cycles over the digests): the product's
    // uniform case 11 (97) and the config-2 case 4 (99)
    case 97: launch_shape<2, 2, (kSplit8V & ~kVCoop) | kVProbe, 2>(A, (groups + 1) / 2, st); break;
    case 99: launch_shape<4, 1, kSplitV<4> | kVProbe, kSplitNProd<4>>(A, groups, st); break;
    case 417:  // the quad shape (product case 416) with the consumer probe: row 16 w of workgroup w
        launch_shape<4, 1, kSplitQuadV | kVProbe, 2>(A, (A.n + 15u) / 16u, st);
        break;
    case 816:  // the quad shape with 8-block units (80 KiB ring, one consumer barrier per 8 blocks)
        launch_shape<8, 1, kSplitQuadV, 2>(A, (A.n + 15u) / 16u, st);
        break;
    case 817:  // ... with the consumer probe
        launch_shape<8, 1, kSplitQuadV | kVProbe, 2>(A, (A.n + 15u) / 16u, st);
        break;
    case 13:  // the product's case 11 with lane-per-chunk producer loads on any layout
        launch_shape<2, 2, kSplit8V & ~kVCoop, 2>(A, (groups + 1) / 2, st);
        break;
    // one pair per workgroup, 2-block units, two producers (waves 0, 1, 3 as in
    // case 4): the config-2 layout with case 11's unit size
    case 16:
        launch_shape<2, 1, kVWK | kVUnmask | kVSkipWave2 | kVRead10 | kVCoop, 2>(A, groups, st);
        break;
    case 17:  // case 16 with lane-per-chunk producer loads
        launch_shape<2, 1, kVWK | kVUnmask | kVSkipWave2 | kVRead10, 2>(A, groups, st);
        break;
    case 8:  // 4 pairs per workgroup (512 threads), one consumer + producer per SIMD
        launch_shape<1, 4>(A, (groups + 3) / 4, st);
        break;
    case 86:  // case 8 with shared producer loads
        launch_shape<1, 4, kVWK | kVUnmask | kVCoop>(A, (groups + 3) / 4, st);
        break;
    case 87:  // case 86 with K added in the consumer
        launch_shape<1, 4, kVUnmask | kVCoop>(A, (groups + 3) / 4, st);
        break;
    case 10:  // 2 pairs x (consumer + 2 producers), 2-block units, 8-wave layout
        launch_shape<2, 2, kVWK | kVUnmask | kVLayout8, 2>(A, (groups + 1) / 2, st);
        break;
    case 12:  // case 10 with schedule reads in bursts of 10
        launch_shape<2, 2, kVWK | kVUnmask | kVLayout8 | kVRead10, 2>(A, (groups + 1) / 2, st);
        break;
    case 9:  // 2 pairs per workgroup, 2-block units
        launch_shape<2, 2>(A, (groups + 1) / 2, st);
        break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
