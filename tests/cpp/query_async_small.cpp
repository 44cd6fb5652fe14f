// tests/cpp/query_async.cpp with room for four ids in an update's AABB ticket: the capacity overflow of the shim's asynchronous
// queries (a request whose lists need more is asked again with the reported total and arrives one update later, complete).
#define EDYN_QUERY_IDS_CAPACITY 4
#include "query_async.cpp"
