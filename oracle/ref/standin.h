/* What oracle/ref/entry.cpp needs from oracle/ref/standin.cpp -- TEST INFRASTRUCTURE ONLY. */
#ifndef HZ_REF_STANDIN_H
#define HZ_REF_STANDIN_H

#include <embree4/rtcore.h>

#include <stdexcept>
#include <string>

namespace hzref {

/* more rays than hzref_set_ray_budget allows: the reference's search would not have ended */
struct budget_exceeded : std::runtime_error {
    budget_exceeded() : std::runtime_error("ray budget exceeded") {}
};

/* the reference asked the stand-in for something the oracle does not model, or its index buffer is not the
 * topology the oracle assumes */
struct standin_error : std::runtime_error {
    explicit standin_error(const std::string &what) : std::runtime_error(what) {}
};

/* devices, scenes and geometries are tracked until they are released; after an exception cut a reference function
 * short, release_leftovers() frees all that are still tracked.  A Terrain's device and scene live on between
 * calls: forget_*() takes them off the list (their owner releases them). */
void release_leftovers();
void forget_scene(RTCScene s);
void forget_device(RTCDevice d);

}  // namespace hzref

#endif
