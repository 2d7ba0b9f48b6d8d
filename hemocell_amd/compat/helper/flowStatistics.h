#pragma once
#include "../flowStatistics.h"
