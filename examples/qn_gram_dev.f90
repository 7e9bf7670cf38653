!  qn_gram_dev -- qn_logpdf_dev's loop (the reference's test/driver2.f90:66-195 on device buffers, the library's
!  built-in separable bounded quadratic, classic entry setulb_dev), then three draws from N(0, H) at the last
!  iterate (lbfgsb_qn_draw, seed 1, samples 0 to 2, no mean, scale 1) and their 3 x 3 Gram matrices around their
!  mean, under B and under H (lbfgsb_qn_gram): g(a, b) = (x_a - xbar)' A (x_b - xbar).  The mean is formed on the
!  host and handed in as the center.
!
!     qn_gram_dev [n [m [iterations]]]      defaults 100000, 5, 12
!
!  Output: one "Iterate" line per iterate, then
!     QNGRAM col = <stored pairs>
!     QNGRAM B <row a of the matrix under B>        (three lines)
!     QNGRAM H <row a of the matrix under H>        (three lines)
      program qn_gram_dev

      use lbfgsb_module, wp => lbfgsp_wp
      use iso_c_binding
      use iso_fortran_env, only: output_unit

      implicit none

      interface
         function hipMalloc(ptr, nbytes) bind(C, name='hipMalloc') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr) :: ptr
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMalloc
         function hipFree(ptr) bind(C, name='hipFree') result(rc)
            import :: c_ptr, c_int
            type(c_ptr), value :: ptr
            integer(c_int) :: rc
         end function hipFree
         function hipMemcpy(dst, src, nbytes, kind) bind(C, name='hipMemcpy') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst, src
            integer(c_size_t), value :: nbytes
            integer(c_int), value :: kind
            integer(c_int) :: rc
         end function hipMemcpy
         function hipMemset(dst, val, nbytes) bind(C, name='hipMemset') result(rc)
            import :: c_ptr, c_size_t, c_int
            type(c_ptr), value :: dst
            integer(c_int), value :: val
            integer(c_size_t), value :: nbytes
            integer(c_int) :: rc
         end function hipMemset
      end interface
      integer(c_int), parameter :: H2D = 1, D2H = 2

      integer               :: n, m, maxit, rc, i
      real(wp), parameter   :: factr = 0.0_wp, pgtol = 0.0_wp
      character(len=60)     :: task, csave
      character(len=32)     :: arg
      logical               :: lsave(4)
      integer               :: isave(44)
      real(wp)              :: f, dsave(29)
      real(c_double)        :: gb(3, 3), gh(3, 3)
      type(c_ptr)           :: ctx, dx, dg, dl, du, dnbd, ddh, dmean
      real(wp), allocatable, target :: hdraw(:)
      integer               :: a
      real(wp), allocatable, target :: hbuf(:)
      integer(c_int32_t), allocatable, target :: hnbd(:)
      integer(c_size_t)     :: vbytes

      n = 100000; m = 5; maxit = 12
      if (command_argument_count() >= 1) then
         call get_command_argument(1, arg); read (arg, *) n
      end if
      if (command_argument_count() >= 2) then
         call get_command_argument(2, arg); read (arg, *) m
      end if
      if (command_argument_count() >= 3) then
         call get_command_argument(3, arg); read (arg, *) maxit
      end if

      vbytes = int(n, c_size_t)*int(storage_size(1.0_wp)/8, c_size_t)
      call chk(hipMalloc(dx, vbytes), 'hipMalloc x')
      call chk(hipMalloc(dg, vbytes), 'hipMalloc g')
      call chk(hipMalloc(dl, vbytes), 'hipMalloc l')
      call chk(hipMalloc(du, vbytes), 'hipMalloc u')
      call chk(hipMalloc(ddh, 3_c_size_t*vbytes), 'hipMalloc draws')
      call chk(hipMalloc(dmean, vbytes), 'hipMalloc mean')
      call chk(hipMalloc(dnbd, int(n, c_size_t)*4_c_size_t), 'hipMalloc nbd')
      call chk(hipMemset(dx, 0_c_int, vbytes), 'hipMemset x')             ! x0 = 0
      call chk(hipMemset(dg, 0_c_int, vbytes), 'hipMemset g')
      allocate (hbuf(n))
      hbuf = -1.0_wp                                                       ! l = -1
      call chk(hipMemcpy(dl, c_loc(hbuf), vbytes, H2D), 'hipMemcpy l')
      hbuf = 1.0_wp                                                        ! u = +1
      call chk(hipMemcpy(du, c_loc(hbuf), vbytes, H2D), 'hipMemcpy u')
      allocate (hnbd(n))
      do i = 1, n
         hnbd(i) = int(mod(i, 4), c_int32_t)                               ! all four bound types
      end do
      call chk(hipMemcpy(dnbd, c_loc(hnbd), int(n, c_size_t)*4_c_size_t, H2D), 'hipMemcpy nbd')
      deallocate (hnbd)

      call lbfgsb_create(ctx, n, m, 0, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_create failed: ', lbfgsb_error_message()
         error stop 1
      end if

      task = 'START'
      f = 0.0_wp
      do while (task(1:2) == 'FG' .or. task == 'NEW_X' .or. task == 'START')
         call setulb_dev(ctx, dx, dl, du, dnbd, f, dg, factr, pgtol, task, -1, csave, lsave, isave, dsave, rc)
         if (rc /= 0) then
            write (output_unit, '(2a)') ' setulb_dev failed: ', lbfgsb_error_message()
            error stop 1
         end if
         if (task(1:2) == 'FG') then
            call lbfgsb_objective(ctx, 0, dx, dg, rc, f)
            if (rc /= 0) error stop 2
         else if (task(1:5) == 'NEW_X') then
            write (output_unit, '(2(a,i5,4x),a,1p,d12.5,4x,a,1p,d12.5)') 'Iterate', isave(30), 'nfg =', isave(34), &
               'f =', f, '|proj g| =', dsave(13)
            if (isave(30) >= maxit) exit                                   ! the model of this NEW_X return
         end if
      end do

      ! three draws from N(0, H), their mean on the host, then the Gram matrices around it under B and under H
      call lbfgsb_qn_draw(ctx, LBFGSB_QN_H, 3, 1_c_int64_t, 0, c_null_ptr, 1.0_c_double, ddh, n, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_draw failed: ', lbfgsb_error_message()
         error stop 1
      end if
      allocate (hdraw(3*n))
      call chk(hipMemcpy(c_loc(hdraw), ddh, 3_c_size_t*vbytes, D2H), 'hipMemcpy draws')
      do i = 1, n
         hbuf(i) = (hdraw(i) + hdraw(n + i) + hdraw(2*n + i))/3.0_wp
      end do
      call chk(hipMemcpy(dmean, c_loc(hbuf), vbytes, H2D), 'hipMemcpy mean')
      deallocate (hdraw)
      call lbfgsb_qn_gram(ctx, LBFGSB_QN_B, 3, ddh, n, dmean, gb, 3, rc)
      if (rc == 0) call lbfgsb_qn_gram(ctx, LBFGSB_QN_H, 3, ddh, n, dmean, gh, 3, rc)
      if (rc /= 0) then
         write (output_unit, '(2a)') ' lbfgsb_qn_gram failed: ', lbfgsb_error_message()
         error stop 1
      end if
      write (output_unit, '(a,i4)') 'QNGRAM col =', isave(28)
      do a = 1, 3
         write (output_unit, '(a,3es25.16e3)') 'QNGRAM B', gb(a, 1), gb(a, 2), gb(a, 3)
      end do
      do a = 1, 3
         write (output_unit, '(a,3es25.16e3)') 'QNGRAM H', gh(a, 1), gh(a, 2), gh(a, 3)
      end do

      task = 'STOP: QN_GRAM_DEV'
      call lbfgsb_destroy(ctx)
      rc = hipFree(dx); rc = hipFree(dg); rc = hipFree(dl); rc = hipFree(du)
      rc = hipFree(ddh); rc = hipFree(dnbd); rc = hipFree(dmean)

      contains

      subroutine chk(code, what)
      integer(c_int), intent(in) :: code
      character(len=*), intent(in) :: what
      if (code /= 0) then
         write (output_unit, '(3a,i0)') ' ', what, ' failed, hipError ', code
         error stop 3
      end if
      end subroutine chk

      end program qn_gram_dev
