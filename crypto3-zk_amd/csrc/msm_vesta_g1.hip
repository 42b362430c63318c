// Pippenger MSM instantiated for one (curve, group): see msm_core.hpp (the kernels that touch coordinates + per-call logic), msm_entries.hpp (the field-free entries stage, compiled once) and msm.hip (dispatch).
#include "msm_core.hpp"

const MsmOps *zk_msm_ops_vesta_g1() { return msm_make_ops<zkhip::CurveTraits<zkhip::CURVE_VESTA, zkhip::GROUP_G1>::F>(); }
