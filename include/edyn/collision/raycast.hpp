// Forwarding header of the MI355X stepper shim: the reference splits its API over many headers, the shim keeps it in one.
// Code that includes <edyn/collision/raycast.hpp> (as code written against the reference does) gets the shim's declarations:
// edyn::raycast, raycast_result and the shape raycast info types.
#ifndef EDYN_HIP_FWD_COLLISION_RAYCAST_HPP
#define EDYN_HIP_FWD_COLLISION_RAYCAST_HPP
#include <edyn/edyn.hpp>
#endif
