// Forwarding header of the MI355X stepper shim: the reference splits its API over many headers, the shim keeps it in one.
// Code that includes <edyn/collision/query_aabb.hpp> (as code written against the reference does) gets the shim's declarations:
// edyn::query_procedural_aabb, edyn::query_non_procedural_aabb and query_aabb_result.
#ifndef EDYN_HIP_FWD_COLLISION_QUERY_AABB_HPP
#define EDYN_HIP_FWD_COLLISION_QUERY_AABB_HPP
#include <edyn/edyn.hpp>
#endif
