// compat forwarding header: the reference's drivers include helper/voxelizeDomain.h by its file name alone
#pragma once
#include "helper/voxelizeDomain.h"
