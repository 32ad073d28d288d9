# -*- coding: utf-8 -*-
__all__ = []
