/* oracle/shim/json/reader.h — TEST INFRASTRUCTURE: the whole stand-in lives in json/json.h (see there). */
#pragma once
#include "json.h"
